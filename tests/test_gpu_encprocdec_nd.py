"""EncProcDec on 1-D and 3-D grids on the GPU: the n-D input pack (nps_pack_grid_input_nd), the encoder and decoder
module boundaries, whole models in inference and in grad mode, processor lists, a two-step rollout and the refusals.

References: the reference's own recorded models (tests/golden/encprocdec_nd.pt) and, at the shapes and processors
the fixture does not cover, the CPU restatement tests/encprocdec_nd_ref.py, which test_encprocdec_nd_host.py pins to
that fixture.  Criteria: the pack is a copy, so exact; outputs rel-L2 < 1e-5 (the project's fp32 bar);
parameter gradients under the rule of tests/test_gpu_unet3d_train.py (encprocdec_nd_ref.grads_ok).
"""
import functools
import types

import pytest
import torch
from torch import nn

from conftest import rel_l2
import encprocdec_nd_ref as R
from encprocdec_nd_ref import golden_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5

# ------------------------------------------------------------------ the pack
SPATIAL = {(1, 40): (40,), (1, 64): (64,), (1, 240): (240,),
           (2, 40): (5, 8), (2, 64): (8, 8), (2, 240): (12, 20),
           (3, 40): (2, 4, 5), (3, 64): (4, 4, 4), (3, 240): (4, 6, 10)}


def _pack_case(P, N, K, S, B=2, c=2, tw=3):
    spatial = SPATIAL[(P, N)]
    g = torch.Generator().manual_seed(1000 * P + N + 10 * K + S)
    u = torch.randn(B, c, tw, *spatial, generator=g)
    pos = torch.rand(B, *spatial, P, generator=g)
    cond = torch.randn(B, K, generator=g) if K else None
    sc = torch.randn(B, S, *spatial, generator=g) if S else None
    n = c * tw + P + K + S
    Cp = (n + 3) // 4 * 4
    vparts = ([cond.reshape(B, K, *([1] * P)).expand(B, K, *spatial)] if K else []) + ([sc] if S else [])
    xin_ref = torch.cat([u.flatten(1, 2), pos.movedim(-1, 1)] + vparts + [torch.zeros(B, Cp - n, *spatial)], dim=1)
    xin_ref = xin_ref.movedim(1, -1).reshape(B, N, Cp)
    vb_ref = torch.cat(vparts, dim=1).movedim(1, -1).reshape(B, N, K + S) if K + S else None
    return spatial, u, pos, cond, sc, Cp, xin_ref, vb_ref


@pytest.mark.parametrize("K,S", [(0, 0), (3, 0), (0, 1), (3, 1)])
@pytest.mark.parametrize("N", [40, 64, 240])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_pack_nd_exact(P, N, K, S):
    """xin = [u | pos(P) | cond | spatial cond | zeros] and vb = [cond | spatial cond] over the flat pixels, against
    torch.cat: N = 40 (one ragged block), 64 (one full block), 240 (three blocks and a tail of 48); c*tw = 6, so the
    12 (P, K, S) combinations pad Cp with 0 to 3 zero channels.  At P = 2 also bit-identical to nps_pack_grid_input."""
    from nps_hip import ops, lib, ptr, stream_ptr, check
    spatial, u, pos, cond, sc, Cp, xin_ref, vb_ref = _pack_case(P, N, K, S)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    ud, posd, condd, scd = dev(u), dev(pos), dev(cond), dev(sc)
    xin, vb = ops.pack_grid_input(ud, posd, condd, scd, Cp)
    B = u.shape[0]
    assert xin.shape == ((B,) + spatial + (Cp,) if P == 2 else (B, N, Cp))
    assert torch.equal(xin.reshape(B, N, Cp).cpu(), xin_ref)
    n = 6 + P + K + S
    assert (xin.reshape(B, N, Cp)[:, :, n:] == 0).all()
    if K + S == 0:
        assert vb is None
    else:
        assert torch.equal(vb.reshape(B, N, K + S).cpu(), vb_ref)
    if P == 2:
        x2 = torch.full((B,) + spatial + (Cp,), float("nan"), device=DEV)
        v2 = torch.full((B,) + spatial + (max(K + S, 1),), float("nan"), device=DEV)
        check(lib.nps_pack_grid_input(ptr(ud), ptr(posd), ptr(condd), ptr(scd), ptr(x2), ptr(v2), B, 6, spatial[0],
                                      spatial[1], K, S, Cp, stream_ptr()), "pack_grid_input")
        assert torch.equal(x2, xin)
        assert torch.equal(v2, vb) if K + S else torch.isnan(v2).all()


def test_pack_nd_1d_pos_without_a_channel_axis():
    from nps_hip import ops
    spatial, u, pos, cond, sc, Cp, xin_ref, _ = _pack_case(1, 240, 3, 1)
    xin, _ = ops.pack_grid_input(u.to(DEV), pos[..., 0].contiguous().to(DEV), cond.to(DEV), sc.to(DEV), Cp)
    assert torch.equal(xin.cpu(), xin_ref)


@pytest.mark.parametrize("P", [0, 4])
def test_pack_nd_refuses_other_position_counts(P):
    """An error from the host checks, not a launch: the output buffer is untouched."""
    from nps_hip import ops, lib, ptr, stream_ptr
    u = torch.zeros(1, 6, 64, device=DEV)
    pos = torch.zeros(1, 64, max(P, 1), device=DEV)
    xin = torch.full((1, 64, 12), float("nan"), device=DEV)
    rc = lib.nps_pack_grid_input_nd(ptr(u), ptr(pos), None, None, ptr(xin), None, 1, 6, 64, P, 0, 0, 12, stream_ptr())
    msg = lib.nps_last_error().decode()
    torch.cuda.synchronize()
    assert rc < 0 and f"P={P}" in msg, (rc, msg)
    assert torch.isnan(xin).all()
    if P == 4:
        with pytest.raises(RuntimeError, match="P=4"):
            ops.pack_grid_input(torch.zeros(1, 2, 3, 64, device=DEV), pos, None, None, 12)


# ------------------------------------------------------------------ module boundaries
GRIDS = {"1d_72": (72,), "1d_96_folded": (96,), "3d": (4, 6, 10)}


@pytest.mark.parametrize("train", [False, True], ids=["inference", "grad_mode"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_elementwise_forward(grid, train):
    """ElementWise.forward on (B, c, tw, *spatial): 1-D at L = 72 (the 1 x L image) and L = 96 (folded into 32-point
    rows), 3-D at (4, 6, 10); n_cond = 2 broadcast channels."""
    from models.enc_proc_dec_components.enc_grid import ElementWise
    spatial = GRIDS[grid]
    nd = len(spatial)
    torch.manual_seed(5)
    m = ElementWise(pde=None, num_c=2, num_spatial_dims=nd, time_window=5, hidden_features=16, n_cond=2,
                    activation=nn.GELU())
    g = torch.Generator().manual_seed(6)
    u = torch.rand(2, 2, 5, *spatial, generator=g)
    pos = torch.rand(2, *spatial, nd, generator=g)
    vb = torch.rand(2, 2, *spatial, generator=g)
    with torch.no_grad():
        ref = R.encoder(m.state_dict(), "", u, pos, vb)
    m = m.to(DEV)
    with torch.set_grad_enabled(train):
        y = m(u.to(DEV), pos.to(DEV), variables_broadcast=vb.to(DEV))
    assert y.shape == ref.shape and y.requires_grad == train
    err = rel_l2(y, ref)
    print(f"ElementWise {grid} {'grad' if train else 'inference'}: rel-L2 {err:.2e}")
    assert err < TOL


@pytest.mark.parametrize("train", [False, True], ids=["inference", "grad_mode"])
@pytest.mark.parametrize("grid,num_c,tw", [("1d_72", 2, 5), ("1d_96_folded", 2, 5), ("3d", 1, 25), ("3d", 3, 25)])
def test_timeconvdense_forward(grid, num_c, tw, train):
    """TimeConvDense.forward on (B, hidden, *spatial): the generic decode kernel (tw = 5) in 1-D, the <1, 25> and
    <3, 25> fast kernels in 3-D; dt = 0.3 so that the delta, not the copied last step, dominates the output."""
    from models.enc_proc_dec_components.dec_grid import TimeConvDense
    spatial = GRIDS[grid]
    nd = len(spatial)
    torch.manual_seed(7)
    m = TimeConvDense(pde=types.SimpleNamespace(dt=0.3), num_c=num_c, num_spatial_dims=nd, time_window=tw,
                      hidden_features=16, activation=nn.GELU())
    g = torch.Generator().manual_seed(8)
    h = torch.randn(2, 16, *spatial, generator=g)
    u = torch.rand(2, num_c, tw, *spatial, generator=g)
    with torch.no_grad():
        ref = R.decoder(m.state_dict(), "", h, u, 0.3)
    m = m.to(DEV)
    with torch.set_grad_enabled(train):
        y = m(h.to(DEV), u.to(DEV))
    assert y.shape == u.shape and y.requires_grad == train
    err = rel_l2(y, ref)
    print(f"TimeConvDense {grid} c={num_c} tw={tw} {'grad' if train else 'inference'}: rel-L2 {err:.2e}")
    assert err < TOL


# ------------------------------------------------------------------ whole models
def _build(kwargs, pde, seed=42, wrapper=None):
    import models
    kw = {k: (tuple(v) if k == "fno_modes" and isinstance(v, list) else v) for k, v in kwargs.items()}
    torch.manual_seed(seed)
    stub = types.SimpleNamespace(**pde)
    if wrapper is not None:
        return models.activation_wrapper(model_class="EncProcDec", pde=stub, activation=nn.GELU(), **wrapper, **kw)
    return models.EncProcDec(pde=stub, activation=nn.GELU(), **kw)


def _call(m, x, cond, pos, sc):
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return m(dev(x), cond=dev(cond), bc=None, pos=dev(pos), t_cond=None, spatial_cond=dev(sc))


@functools.lru_cache(maxsize=None)
def _golden_model(name):
    g = golden_case(name)
    m = _build(g["kwargs"], g["pde"])
    m.load_state_dict(g["state_dict"])
    return g, m.to(DEV)


@pytest.mark.parametrize("name", ["epd1d_fno", "epd3d_fno"])
def test_golden_model_inference(name):
    g, m = _golden_model(name)
    with torch.no_grad():
        y = _call(m, g["x"], g["cond"], g["pos"], g.get("spatial_cond"))
    err = rel_l2(y, g["y"])
    print(f"{name} inference: y rel-L2 {err:.2e}")
    assert y.shape == g["y"].shape and not y.requires_grad and err < TOL


@pytest.mark.parametrize("name", ["epd1d_fno", "epd3d_fno"])
def test_golden_model_trains(name):
    g, m = _golden_model(name)
    for p in m.parameters():
        p.grad = None
    y = _call(m, g["x"], g["cond"], g["pos"], g.get("spatial_cond"))
    err = rel_l2(y, g["y"])
    print(f"{name} grad mode: y rel-L2 {err:.2e}")
    assert y.requires_grad and err < TOL
    y.backward(g["g"].to(DEV))
    got = {k: p.grad for k, p in m.named_parameters()}
    assert set(got) == set(g["grads"])
    R.grads_ok(g["grads"], got)


UNET1 = dict(hidden_features=16, cond_mode="concat", norm=True, ch_mults=[1], n_blocks=1, use1x1=False,
             padding_mode="circular")                                   # test_gpu_unet3d_train.UNET1
FNO_CFG = dict(hidden_blocks=2, fno_modes=(3, 4, 3), fno_kernel_size=1, fno_conv_mode="single")
BASE3D = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", num_spatial_dims=3, num_c=3,
              time_window=25)
PDE3D = dict(dt=0.1, n_cond_static=2, n_cond_spatial=0)
VOL = (6, 7, 9)  # N = 378: 23 decode groups of 16 and a tail of 10; 5 pack blocks and a tail of 58
MODELS3D = {
    # (the U-FNO's U-Nets end in a 1x1x1 conv, as that file's one-level "ufno1")
    "UFNO": dict(BASE3D, processor="UFNO", **dict(UNET1, use1x1=True), **FNO_CFG),
    "UNetModern": dict(BASE3D, processor="UNetModern", **UNET1),
    "FNO_UFNO_residual": dict(BASE3D, processor=[dict(object="FNO"), dict(object="UFNO")], processor_residual=True,
                              **dict(UNET1, use1x1=True), **FNO_CFG),
}


def _inputs3d(num_c=3, n_static=2, seed=21, B=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, num_c, 25, *VOL, generator=g)
    cond = torch.rand(B, n_static, generator=g)
    axes = torch.meshgrid(*[torch.linspace(0, 1, s) for s in VOL], indexing="ij")
    pos = torch.stack(axes, dim=-1)[None].repeat(B, 1, 1, 1, 1).contiguous()
    gy = torch.randn(B, num_c, 25, *VOL, generator=g)
    return x, cond, pos, gy


@functools.lru_cache(maxsize=None)
def _model3d(name):
    """The model, its inputs and the fp64 restatement (output and gradients) of one MODELS3D entry, built once."""
    m = _build(MODELS3D[name], PDE3D, seed=9)
    x, cond, pos, gy = _inputs3d()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert set(sd) == set(dict(m.named_parameters()))
    ref_y, ref_grads = R.reference_grads(sd, MODELS3D[name], PDE3D, x, cond, pos, None, gy)
    return m.to(DEV), (x, cond, pos, gy), ref_y, ref_grads


@pytest.mark.parametrize("name", list(MODELS3D))
def test_model3d_inference_vs_restatement(name):
    m, (x, cond, pos, _), ref_y, _ = _model3d(name)
    with torch.no_grad():
        y = _call(m, x, cond, pos, None)
    err = rel_l2(y, ref_y)
    print(f"3-D {name} inference: y rel-L2 {err:.2e}")
    assert y.shape == x.shape and err < TOL


@pytest.mark.parametrize("name", ["UFNO", "UNetModern"])
def test_model3d_trains_vs_restatement(name):
    m, (x, cond, pos, gy), ref_y, ref_grads = _model3d(name)
    for p in m.parameters():
        p.grad = None
    y = _call(m, x, cond, pos, None)
    err = rel_l2(y, ref_y)
    print(f"3-D {name} grad mode: y rel-L2 {err:.2e}")
    assert y.requires_grad and err < TOL
    y.backward(gy.to(DEV))
    R.grads_ok(ref_grads, {k: p.grad for k, p in m.named_parameters()})


def test_rollout_two_steps_with_final_tanh():
    """activation_wrapper(Tanh) around the 3-D FNO model of the fixture (with its spatial_cond input channel): two
    autoregressive calls, the second on the GPU's own first output; each step against the restatement given the same
    input (the BASELINE.md parity rule: per step, no compounding)."""
    g = golden_case("epd3d_fno")
    m = _build(g["kwargs"], g["pde"], wrapper=dict(activation_final=nn.Tanh()))
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV).eval()
    assert type(m).__name__ == "ActWrapper-EncProcDec"
    x = g["x"]
    for step in range(2):
        with torch.no_grad():
            y = _call(m, x, g["cond"], g["pos"], g["spatial_cond"]).cpu()
            ref = R.encprocdec_nd(g["state_dict"], g["kwargs"], g["pde"], x, g["cond"], g["pos"], g["spatial_cond"],
                                  final_tanh=True)
        err = rel_l2(y, ref)
        print(f"rollout step {step}: rel-L2 {err:.2e}")
        assert err < TOL and y.abs().max() <= 1.0
        x = y


# ------------------------------------------------------------------ refusals
# The models live on the GPU and the inputs stay on the CPU: the first launch (or its is_cuda check) would raise a
# RuntimeError about the device, so the NotImplementedError / ValueError below shows the refusal comes before it.
@pytest.mark.parametrize("nd,processor,extra,match", [
    (3, "DilatedResnet", dict(kernel_size=3, hidden_blocks=1, padding_mode="circular"), "DilatedResnet.*3-D"),
    (1, "DilatedResnet", dict(kernel_size=3, hidden_blocks=1, padding_mode="circular"), "DilatedResnet.*1-D"),
    (1, "UFNO", dict(UNET1, use1x1=True, hidden_blocks=1, fno_modes=3), "UFNO.*1-D"),
    (1, "UNetModern", dict(UNET1), "UNetModern.*1-D"),
])
def test_processors_without_a_path_are_refused(nd, processor, extra, match):
    spatial = (64,) if nd == 1 else (4, 4, 4)
    kw = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", num_spatial_dims=nd, num_c=1,
              time_window=5, processor=processor, **dict(dict(hidden_features=16), **extra))
    m = _build(kw, dict(dt=0.1, n_cond_static=0, n_cond_spatial=0)).to(DEV)
    x = torch.rand(1, 1, 5, *spatial)
    pos = torch.rand(1, *spatial, nd)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match=match):
            m(x, pos=pos)


def test_supported_model_with_cpu_inputs_reaches_the_device_check():
    """The control of the refusal tests: a model that has a path fails on the CPU inputs instead."""
    g, m = _golden_model("epd1d_fno")
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        m(g["x"], cond=g["cond"], pos=g["pos"])


def test_wrapper_refusals_off_the_2d_grid():
    g = golden_case("epd3d_fno")
    x, cond, pos, sc = (g[k] for k in ("x", "cond", "pos", "spatial_cond"))
    m = _build(g["kwargs"], g["pde"], wrapper=dict(activation_final=nn.Tanh(), enforce_spatial_cond=True)).to(DEV)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="enforce_spatial_cond.*2-D"):
        m(x, cond=cond, pos=pos, spatial_cond=sc)
    m = _build(g["kwargs"], g["pde"], wrapper=dict(activation_final=nn.Tanh(), approx_volume_preserve=True,
                                                   approx_volume_preserve_mode="individual_static")).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="3 spatial dims not supported for approx volume preserve"):
        m(x, cond=cond, pos=pos, spatial_cond=sc)
    g1 = golden_case("epd1d_fno")
    m = _build(g1["kwargs"], g1["pde"], wrapper=dict(activation_final=nn.Tanh(), approx_volume_preserve=True)).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="1 spatial dims not supported"):
        m(g1["x"], cond=g1["cond"], pos=g1["pos"])
