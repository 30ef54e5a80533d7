"""U-Net attention on the GPU: nps_attn_colstats / nps_attn_fwd / nps_attn_bwd through ctypes against the fp64
closed form (tests/test_attention_host.py: attention_core_fp64, softmax over the QUERY index), the modules
against the reference fixtures tests/golden/attention.pt (a, b, c) and attention_model.pt (d).

The kernels work on 64-row tiles (queries and keys alike) and 64-wide head-dimension chunks, so the cases
(B, N, heads, dk) sit on and around those sizes:
  (1, 1, 1, 4)       one token, the smallest dk: a single row and column of one tile, 60 padded chunk columns
  (2, 63, 1, 8)      one row short of a tile
  (1, 64, 2, 20)     exactly one tile; two heads (q/k/v column offsets inside a token), dk no multiple of 16
  (3, 65, 3, 12)     one row into the second tile: 63 padded queries AND 63 padded keys in the last tile pair
  (1, 128, 1, 64)    exactly two tiles and exactly one chunk
  (1, 70, 2, 68)     dk four columns into the second chunk
  (1, 127, 1, 132)   three chunks, the last partial; one row short of two tiles
  (1, 193, 1, 192)   three full chunks (the C2/C3 mid-level width), one row into the fourth tile
  (2, 130, 1, 256)   the largest dk (four chunks), two rows into the third tile
  (1, 3481, 1, 192)  the C2 mid level (59 x 59 tokens): 55 tiles, the online column max / sum over many steps
Outputs, lse and dqkv are written between NaN guard rows (one batch row before and after), so a store outside
[0, B) x [0, N) x the channel range shows; the kernels write every element inside, so no NaN may remain there.
"""
import pytest
import torch
from torch import nn

from conftest import load_golden, rel_l2
from test_attention_host import attention_core_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5

CASES = [(1, 1, 1, 4), (2, 63, 1, 8), (1, 64, 2, 20), (3, 65, 3, 12), (1, 128, 1, 64), (1, 70, 2, 68),
         (1, 127, 1, 132), (1, 193, 1, 192), (2, 130, 1, 256), (1, 3481, 1, 192)]


def _guarded(B, *shape):
    return torch.full((B + 2,) + shape, float("nan"), device=DEV)


def _inner(buf, what):
    B = buf.shape[0] - 2
    assert buf[0].isnan().all() and buf[B + 1].isnan().all(), f"{what}: wrote outside its tensor"
    assert torch.isfinite(buf[1:B + 1]).all(), f"{what}: non-finite or unwritten elements"
    return buf[1:B + 1]


def _cancellation_norms(qkv64, dout64, heads, dk, scale):
    """dS[i][j] = P[i][j] (dp[i][j] - delta[j]) is a difference; where it cancels (one query holding nearly all of
    a column, or N = 1 where it is identically 0) dQ and dK are far smaller than the terms they are made of and no
    fp32 evaluation resolves them relative to themselves.  These are the norms of the term-wise magnitudes
    scale sum P (|dp| + |delta|) |k| and scale sum P (|dp| + |delta|) |q| — what fp32 rounding is relative to."""
    B, N = qkv64.shape[:2]
    q, k, v = torch.chunk(qkv64.view(B, N, heads, 3 * dk), 3, dim=-1)
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    p = torch.exp(s - torch.logsumexp(s, dim=2, keepdim=True))
    dp = torch.einsum("bihd,bjhd->bhij", dout64.view(B, N, heads, dk), v)
    c = p * (dp.abs() + (p * dp).sum(2, keepdim=True).abs())
    return (scale * torch.einsum("bhij,bjhd->bihd", c, k.abs()).norm().item(),
            scale * torch.einsum("bhij,bihd->bjhd", c, q.abs()).norm().item())


def _kernels_vs_fp64(qkv, dout, heads, dk, scale, cancelling=False):
    """Runs the three entry points on fp32 device tensors; returns the rel-L2 errors against fp64.  cancelling:
    dq and dk errors are taken relative to _cancellation_norms instead of the (vanishing) gradients themselves."""
    from nps_hip import lib, ptr, stream_ptr, check
    B, N = qkv.shape[:2]
    lse, out, dqkv = _guarded(B, heads, N), _guarded(B, N, heads * dk), _guarded(B, N, heads * 3 * dk)
    s = stream_ptr()
    check(lib.nps_attn_colstats(ptr(qkv), ptr(lse[1:]), B, N, heads, dk, scale, s), "attn_colstats")
    check(lib.nps_attn_fwd(ptr(qkv), ptr(lse[1:]), ptr(out[1:]), B, N, heads, dk, scale, s), "attn_fwd")
    ws = torch.full((lib.nps_attn_bwd_ws_floats(B, N, heads, dk),), float("nan"), device=DEV)
    check(lib.nps_attn_bwd(ptr(qkv), ptr(lse[1:]), ptr(dout), ptr(dqkv[1:]), ptr(ws), B, N, heads, dk, scale, s),
          "attn_bwd")
    torch.cuda.synchronize()
    q64 = qkv.double().requires_grad_(True)
    o64, l64 = attention_core_fp64(q64, heads, dk, scale)
    (g64,) = torch.autograd.grad(o64, q64, dout.double())
    got = _inner(dqkv, "dqkv").view(B, N, heads, 3, dk)
    want = g64.view(B, N, heads, 3, dk)
    errs = dict(out=rel_l2(_inner(out, "out"), o64), lse=rel_l2(_inner(lse, "lse"), l64))
    for i, part in enumerate(("dq", "dk", "dv")):
        errs[part] = rel_l2(got[:, :, :, i], want[:, :, :, i])
    if cancelling:
        with torch.no_grad():
            cq, ck = _cancellation_norms(qkv.double(), dout.double(), heads, dk, scale)
        errs["dq"] = torch.linalg.vector_norm(got[:, :, :, 0].double() - want[:, :, :, 0]).item() / cq
        errs["dk"] = torch.linalg.vector_norm(got[:, :, :, 1].double() - want[:, :, :, 1]).item() / ck
    return errs


@pytest.mark.parametrize("B,N,heads,dk", CASES)
def test_attention_kernels_vs_fp64(B, N, heads, dk):
    g = torch.Generator().manual_seed(1000 * N + dk)
    qkv = torch.randn(B, N, heads * 3 * dk, generator=g).to(DEV)
    dout = torch.randn(B, N, heads * dk, generator=g).to(DEV)
    # N = 1: the softmax of a single query is the constant 1, so dq = dk = 0 exactly (no rel-L2 against that)
    errs = _kernels_vs_fp64(qkv, dout, heads, dk, dk ** -0.5, cancelling=N == 1)
    print(f"attention B={B} N={N} heads={heads} dk={dk}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


def test_attention_large_logits():
    """q and k scaled so the logits span about +-90 (fp32 exp of the raw logits would overflow at 88.7): the
    column max keeps every exponent <= 0."""
    B, N, heads, dk = 1, 130, 1, 8
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, N, heads, 3, dk, generator=g)
    qkv[:, :, :, :2] *= 4.0   # logit std = 4^2 = 16; the extremes of these 130^2 are -93 and +87
    qkv = qkv.view(B, N, -1).to(DEV)
    dout = torch.randn(B, N, heads * dk, generator=g).to(DEV)
    q, k, _ = torch.chunk(qkv.view(B, N, heads, 3 * dk).double(), 3, dim=-1)
    logits = torch.einsum("bihd,bjhd->bhij", q, k) * dk ** -0.5
    print(f"logit range [{logits.min().item():.1f}, {logits.max().item():.1f}]")
    assert logits.max() > 75 and logits.min() < -75
    errs = _kernels_vs_fp64(qkv, dout, heads, dk, dk ** -0.5)
    print("large logits: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


@pytest.mark.parametrize("lead", [8.0, 60.0])
def test_attention_one_query_dominates_every_column(lead):
    """Every key shares a direction that query 0 points along: column j's softmax is dominated by i = 0, so
    out_0 ~ sum_j v_j.
    lead 8: query 0 holds 88 % of a column on average and at least twice any other query's weight in every
    column; every result is held to rel-L2 < 1e-5.  dS = P (dp - delta) cancels as P[0][j] -> 1, so fp32
    rounding (~1e-7 of the terms) is amplified by cond = |terms| / |gradient| (_cancellation_norms over the
    gradient's norm): about 60 for dq and 14 for dk here, which leaves the bound a margin; at lead 10 the same
    data has cond 250 and no fp32 evaluation of these formulas keeps 1e-5.
    lead 60: the others are ~e^-60; out, lse and dv stay finite and < 1e-5; dq and dk are then differences of
    O(1) terms with true norm ~1e-25, judged against the terms they cancel from."""
    B, N, heads, dk = 2, 100, 1, 16
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, N, heads, 3, dk, generator=g)
    qkv[:, :, :, 1, 0] = 4.0          # every key: component 4 along e_0
    qkv[:, 0, :, 0, 0] = lead         # query 0: logit lead * 4 * dk^-0.5 = lead above the others' mean
    qkv = qkv.view(B, N, -1).to(DEV)
    dout = torch.randn(B, N, heads * dk, generator=g).to(DEV)
    q, k, _ = torch.chunk(qkv.view(B, N, heads, 3 * dk).double(), 3, dim=-1)
    p0 = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * dk ** -0.5, dim=2)[:, :, 0]
    pall = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * dk ** -0.5, dim=2)
    margin = (p0 / pall[:, :, 1:].max(dim=2).values).min().item()
    print(f"lead {lead}: query 0 holds {p0.min().item():.3f} .. {p0.max().item():.3f} of a column, mean "
          f"{p0.mean().item():.3f}, at least {margin:.1f} x any other query")
    assert margin > 2 and p0.mean() > 0.85
    errs = _kernels_vs_fp64(qkv, dout, heads, dk, dk ** -0.5, cancelling=lead > 10.0)
    print("dominant query: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


def test_attention_memory_does_not_grow_as_n_squared():
    """(1, 4096, 1, 64): the score matrix alone would be 64 MiB; forward + backward must stay under 16 MiB."""
    from nps_hip import ops
    B, N, heads, dk = 1, 4096, 1, 64
    qkv = torch.randn(B, N, heads * 3 * dk, device=DEV)
    dout = torch.randn(B, N, heads * dk, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, lse = ops.attention(qkv, heads, dk, dk ** -0.5)
    dqkv = ops.attention_bwd(qkv, lse, dout, heads, dk, dk ** -0.5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"fwd + bwd allocated {grown / 2 ** 20:.2f} MiB beyond the inputs")
    assert grown < 16 * 2 ** 20
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()


# ------------------------------------------------------------------ modules vs the reference fixtures
def _block(name):
    from models.enc_proc_dec_components.proc_unet_modern import AttentionBlock
    g = load_golden("attention")[name]
    m = AttentionBlock(**g["kwargs"])
    m.load_state_dict(g["state_dict"])
    return m.to(DEV), g


def _check_grads(m, want):
    """Every parameter gradient: rel-L2 < 1e-5, or — for a gradient that is a sum over every pixel which cancels
    (a bias or GroupNorm affine; analytically 0 for the last UpBlock's shortcut bias, which feeds the per-channel
    GroupNorm(8, 8)) and which the fp32 reference itself only resolves to rounding noise — an error below
    1e-5 x the norm of the whole gradient (the second clause of tests/test_gpu_backward.py _grads_ok).  All
    gradients as one vector: rel-L2 < 1e-5.  Parameters the reference gives no gradient (the unused attention
    norm) must have none here."""
    got, ref = [], []
    for k, p in m.named_parameters():
        if want[k] is None:
            assert p.grad is None, f"{k} received a gradient"
        else:
            assert p.grad is not None, f"{k} received no gradient"
            got.append(p.grad.detach().cpu().double().reshape(-1))
            ref.append(want[k].double().reshape(-1))
    total = torch.linalg.vector_norm(torch.cat(ref)).item()
    e_all = torch.linalg.vector_norm(torch.cat(got) - torch.cat(ref)).item() / total
    bad = []
    for k, p in m.named_parameters():
        if want[k] is not None:
            err = rel_l2(p.grad, want[k])
            if err >= TOL:
                absolute = torch.linalg.vector_norm(p.grad.detach().cpu().double() - want[k].double()).item()
                print(f"  {k}: rel-L2 {err:.2e}, error / whole gradient {absolute / total:.2e}")
                if not (k.endswith(".bias") or ".norm" in k) or absolute >= TOL * total:
                    bad.append((k, err))
    print(f"parameter gradients as one vector: rel-L2 {e_all:.2e}")
    assert not bad and e_all < TOL, (bad, e_all)


@pytest.mark.parametrize("name", ["a", "b"])
def test_attention_block_golden(name):
    m, g = _block(name)
    with torch.no_grad():
        y = m(g["x"].to(DEV))
    err = rel_l2(y, g["y"])
    print(f"AttentionBlock {name} inference: rel-L2 {err:.2e}")
    assert err < TOL
    x = g["x"].to(DEV).requires_grad_(True)
    y = m(x)
    assert rel_l2(y, g["y"]) < TOL
    y.backward(g["g"].to(DEV))
    assert rel_l2(x.grad, g["dx"]) < TOL
    assert m.norm.weight.grad is None and m.norm.bias.grad is None   # the unused GroupNorm
    _check_grads(m, g["grads"])


def _unet(g):
    from models.enc_proc_dec_components import UNetModern
    m = UNetModern(pde=None, activation=nn.GELU(), **g["kwargs"])
    m.load_state_dict(g["state_dict"])
    return m.to(DEV)


def test_unet_with_attention_fused_inference_golden():
    """norm=True: every ResidualBlock after an attention normalises with the moments its input carries, so
    moments of the attention's INPUT left on its output would show here."""
    g = load_golden("attention")["c"]
    m = _unet(g)
    with torch.no_grad():
        y = m(h=g["h"].to(DEV), variables_broadcast=g["vb"].to(DEV))
        y2 = m(h=g["h"].to(DEV), variables_broadcast=g["vb"].to(DEV))   # cached packings
    err = rel_l2(y, g["y"])
    print(f"UNetModern with attention, fused inference: rel-L2 {err:.2e}")
    assert err < TOL and rel_l2(y2, g["y"]) < TOL


def test_unet_with_attention_autograd_golden():
    g = load_golden("attention")["c"]
    m = _unet(g)
    h = g["h"].to(DEV).requires_grad_(True)
    y = m(h=h, variables_broadcast=g["vb"].to(DEV))
    err = rel_l2(y, g["y"])
    print(f"UNetModern with attention, autograd path: rel-L2 {err:.2e}")
    assert err < TOL
    y.backward(g["g"].to(DEV))
    assert rel_l2(h.grad, g["dh"]) < TOL
    _check_grads(m, g["grads"])


def test_model_with_attention_golden():
    import models
    from pdes import PDE2D
    g = load_golden("attention_model")["d"]
    cfg = dict(g["cfg"], activation=nn.GELU(), activation_final=nn.Tanh())
    p = g["pde"]
    pde = PDE2D(tmin=p["tmin"], tmax=p["tmax"], nt=p["nt"], L1=1.0, L2=1.0, nx1=p["nx1"], nx2=p["nx2"], x=None,
                name="twophase", n_cond_static=p["n_cond_static"], n_cond_spatial=p["n_cond_spatial"])
    m = models.activation_wrapper(**cfg, pde=pde)
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV).eval()
    with torch.no_grad():
        y = m(g["u"].to(DEV), cond=g["cond"].to(DEV), bc=None, pos=g["pos"].to(DEV), t_cond=None,
              spatial_cond=g["spatial_cond"].to(DEV))
    err = rel_l2(y, g["y"])
    print(f"EncProcDec around the attention U-Net, one call: rel-L2 {err:.2e}")
    assert err < TOL


def test_twophase_ufno_with_attention_simulates_and_trains():
    """The twophase U-FNO cfg at reduced width with is_attn=[False, True] and mid_attn=True: a rollout through the
    trainer's simulate, then one training step (forward with grad, sqrt(MSE_sum), backward, Adam) — no
    NotImplementedError, finite numbers, and every attention projection is trained."""
    import argparse
    import types
    import models
    from common.interfaces import D
    from pdes import PDE2D
    from trainers.autoregressivepushforwardtrainer import AutoregressivePushforwardTrainer
    from trainers.synthetic import twophase_batch
    from nps_hip import autograd as ad
    res, tw, T = 32, 25, 75
    pde = PDE2D(tmin=0.0, tmax=1.0, nt=501, L1=1.0, L2=1.0, nx1=res, nx2=res, x=None, name="twophase",
                n_cond_static=3, n_cond_spatial=1)
    cfg = dict(activation_final=nn.Tanh(), enforce_spatial_cond=True, spatial_cond_channel=0,
               approx_volume_preserve=True, approx_volume_preserve_mode="individual_static", max_pct_dif=1 / 25,
               model_class="EncProcDec", num_c=3, num_spatial_dims=2, time_window=tw, data_structure="grid",
               processor_residual=False, encoder="enc_grid.ElementWise", activation=nn.GELU(), processor="UFNO",
               fno_modes=4, hidden_blocks=1, hidden_features=16, fno_kernel_size=1, fno_conv_mode="single",
               padding_mode="circular", ch_mults=[1, 2], is_attn=[False, True], mid_attn=True, norm=True,
               use1x1=True, decoder="dec_grid.TimeConvDense", dec_delta_mode="per_step")
    torch.manual_seed(0)
    m = models.activation_wrapper(**cfg, pde=pde).to(DEV)
    attn = {k: p for k, p in m.named_parameters() if ".attn." in k}
    assert any(".middle.attn." in k for k in attn) and any(".down." in k for k in attn) and any(".up." in k for k in attn)
    u, cond, pos, sc = (t.to(DEV) for t in twophase_batch(B=2, num_c=3, T=T, H=res, W=res, seed=5))
    conf = argparse.Namespace(time_window=tw, base_resolution=(T, res, res), device=DEV, nr_gt_steps=1)
    tr = AutoregressivePushforwardTrainer(model=m.eval(), data=types.SimpleNamespace(pde=pde, data_interface=D.sim2d),
                                          criterion=nn.MSELoss(reduction="sum"), config=conf)
    with torch.no_grad():
        losses, (gt, preds) = tr.simulate(u, cond, pos, compute_loss=True, include_data=True, nr_gt_steps=1, t_res=T,
                                          spatial_conditioning=sc)
    assert all(torch.isfinite(p).all() for p in preds) and all(torch.isfinite(l).all() for l in losses)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    before = {k: p.detach().clone() for k, p in attn.items()}
    pred = m(u[:, :, :tw], cond=cond, bc=None, pos=pos, t_cond=None, spatial_cond=sc)
    loss = ad.sqrt_mse_sum(pred, u[:, :, tw:2 * tw].contiguous())
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    for k, p in attn.items():
        if ".norm." in k:
            assert p.grad is None, k                       # the unused GroupNorm
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
            assert not torch.equal(p.detach(), before[k]), k


def test_3d_attention_still_refused():
    from models.enc_proc_dec_components.proc_unet_modern import AttentionBlock, DownBlock
    with pytest.raises(NotImplementedError):
        AttentionBlock(8)(torch.zeros(1, 8, 4, 4, 4, device=DEV))
    blk = DownBlock(8, 8, has_attn=True, num_spatial_dims=3, padding_kwargs=dict(padding_mode="circular")).to(DEV)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            blk(torch.zeros(1, 8, 4, 4, 4, device=DEV))


def test_unet_without_attention_unchanged():
    """is_attn all False, mid_attn False: the existing `unet_cfg` fixture, asserted as tests/test_gpu_parity.py
    does, with no attention launch on the way."""
    from models.enc_proc_dec_components import UNetModern
    from nps_hip import ops
    g = load_golden("unet_cfg")
    m = UNetModern(pde=None, activation=nn.GELU(), **g["kwargs"])
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV)
    calls = []
    orig = ops.attention
    ops.attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        with torch.no_grad():
            y = m(h=g["h"].to(DEV), variables_broadcast=g["vb"].to(DEV)).cpu()
    finally:
        ops.attention = orig
    assert not calls
    assert y.shape == g["y"].shape
    assert rel_l2(y, g["y"]) < TOL
