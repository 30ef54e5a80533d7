"""U-Net attention, host side (no GPU): what the fixtures in tests/golden/attention.pt pin.

`attention_fp64` below is the test's own restatement of reference proc_unet_modern.py:292-317 in fp64: tokens are
the flattened positions, `norm` is never applied, the per-head layout of the projection is [q | k | v], and the
softmax runs over the QUERY index for each key (dim=1 of [b, i, j, h]).  It must reproduce fixtures (a) and (b) —
outputs and the reference's autograd gradients — so a row softmax, an applied norm or another q/k/v split shows
here before any kernel runs.  tests/test_gpu_attention.py imports it as the modules' and kernels' reference.
"""
import pytest
import torch

from conftest import load_golden, rel_l2


def attention_core_fp64(qkv, heads, dk, scale):
    """qkv (B, N, heads * 3 * dk) fp64 -> (out (B, N, heads * dk), lse (B, heads, N)); softmax over queries."""
    B, N = qkv.shape[:2]
    q, k, v = torch.chunk(qkv.view(B, N, heads, 3 * dk), 3, dim=-1)
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    lse = torch.logsumexp(s, dim=2)                      # over the query index i, per key j
    p = torch.exp(s - lse[:, :, None, :])
    out = torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, N, heads * dk)
    return out, lse


def attention_fp64(sd, x, heads, dk):
    """AttentionBlock forward from a state_dict (fp64 tensors), x (B, C, *spatial).  `norm.*` is unused."""
    B, C = x.shape[:2]
    tok = x.reshape(B, C, -1).permute(0, 2, 1)
    qkv = tok @ sd["projection.weight"].T + sd["projection.bias"]
    o, _ = attention_core_fp64(qkv, heads, dk, dk ** -0.5)
    res = o @ sd["output.weight"].T + sd["output.bias"]
    if "shortcut.weight" in sd:
        w = sd["shortcut.weight"]
        res = res + tok @ w.reshape(w.shape[0], w.shape[1]).T + sd["shortcut.bias"]
    else:
        res = res + tok
    return res.permute(0, 2, 1).reshape(B, -1, *x.shape[2:])


def _meta(kw):
    c = kw["in_channels"]
    return kw.get("n_heads", 1), kw.get("d_k", None) or c


@pytest.mark.parametrize("name", ["a", "b"])
def test_fp64_restatement_reproduces_the_fixture(name):
    g = load_golden("attention")[name]
    heads, dk = _meta(g["kwargs"])
    sd = {k: v.double().requires_grad_(True) for k, v in g["state_dict"].items()}
    x = g["x"].double().requires_grad_(True)
    y = attention_fp64(sd, x, heads, dk)
    assert rel_l2(y, g["y"]) < 1e-6
    y.backward(g["g"].double())
    assert rel_l2(x.grad, g["dx"]) < 1e-6
    for k, want in g["grads"].items():
        if want is None:
            assert k.startswith("norm.") and sd[k].grad is None, k   # the unused GroupNorm
        else:
            assert rel_l2(sd[k].grad, want) < 1e-6, k


def test_a_row_softmax_does_not_reproduce_the_fixture():
    """The usual attention (softmax over keys) is a different function: the fixture tells them apart."""
    g = load_golden("attention")["a"]
    sd = {k: v.double() for k, v in g["state_dict"].items()}
    x = g["x"].double()
    B, C = x.shape[:2]
    tok = x.reshape(B, C, -1).permute(0, 2, 1)
    q, k, v = torch.chunk(tok @ sd["projection.weight"].T + sd["projection.bias"], 3, dim=-1)
    p = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=2)
    res = (p @ v) @ sd["output.weight"].T + sd["output.bias"] + tok
    assert rel_l2(res.permute(0, 2, 1).reshape(x.shape), g["y"]) > 1e-3


@pytest.mark.parametrize("name", ["a", "b"])
def test_seeded_construction_gives_the_fixture_state_dict(name):
    from models.enc_proc_dec_components.proc_unet_modern import AttentionBlock
    g = load_golden("attention")[name]
    torch.manual_seed(42)
    m = AttentionBlock(**g["kwargs"])
    sd = m.state_dict()
    assert list(sd) == list(g["state_dict"])
    for k, v in g["state_dict"].items():
        assert sd[k].shape == v.shape, k
    m.load_state_dict(g["state_dict"])


def test_unet_with_attention_has_the_fixture_state_dict():
    from torch import nn
    from models.enc_proc_dec_components import UNetModern
    g = load_golden("attention")["c"]
    m = UNetModern(pde=None, activation=nn.GELU(), **g["kwargs"])
    m.load_state_dict(g["state_dict"])
    attn = [k for k in g["state_dict"] if ".attn." in k]
    assert any(k.startswith("middle.attn.") for k in attn) and any(k.startswith("down.") for k in attn) \
        and any(k.startswith("up.") for k in attn)


def test_attention_op_refuses_cpu_tensors():
    from nps_hip import ops
    from nps_hip import autograd as ad
    qkv = torch.zeros(1, 5, 12)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.attention(qkv, 1, 4, 0.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ad.attention(qkv, 1, 4, 0.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.attention_bwd(qkv, torch.zeros(1, 1, 5), torch.zeros(1, 5, 4), 1, 4, 0.5)


def test_entry_points_refuse_unsupported_shapes():
    """dk % 4 != 0, dk > 256 and empty sizes are errors through nps_last_error, before any launch."""
    from nps_hip import lib
    for B, N, heads, dk in [(1, 8, 1, 6), (1, 8, 1, 260), (1, 8, 1, 0), (1, 0, 1, 8), (0, 8, 1, 8), (1, 8, 0, 8)]:
        assert lib.nps_attn_colstats(None, None, B, N, heads, dk, 1.0, None) < 0
        assert lib.nps_attn_fwd(None, None, None, B, N, heads, dk, 1.0, None) < 0
        assert lib.nps_attn_bwd(None, None, None, None, None, B, N, heads, dk, 1.0, None) < 0
        assert b"nps_attn_bwd" in lib.nps_last_error()
    assert lib.nps_attn_bwd_ws_floats(2, 100, 3, 8) >= 2 * 100 * 3
