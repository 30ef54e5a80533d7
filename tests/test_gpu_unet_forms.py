"""The U-Net modules' forward() against the hand-written composition of their channels-last entry points, in
each of the three forms (2-D inference, 2-D autograd, 3-D inference), bit for bit; which parameters the
autograd form reaches; the 3-D refusal under autograd; and the whole model's two 2-D forms against each other.

The goldens (tests/test_gpu_parity.py, test_gpu_backward.py, test_gpu_attention.py, test_gpu_ufno3d.py) stay the
pin against the reference: this file pins the module boundaries and the one traversal behind them.
"""
import pytest
import torch
from torch import nn

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5  # tests/test_gpu_backward.py: the autograd path's forward against the same reference as the inference path
PADS = [dict(padding=1), dict(padding_mode="circular")]
PAD_IDS = ["ones", "circular"]

# (kind, constructor args, has_attn, channels of x, channels of vb): 16 -> 16 takes the identity shortcut (one
# source: no conditioning), 20 -> 32 the 1x1 shortcut on a frame whose second source starts off a 16-channel
# boundary (the frame_pack route)
CASES_2D = [
    ("res", (16, 16), None, 16, 0),
    ("res", (20, 32), None, 20, 0),
    ("down", (16, 16), False, 16, 0),
    ("down", (20, 32), True, 16, 4),
    ("middle", (16, 16), False, 16, 0),
    ("middle", (20, 32), True, 16, 4),
    ("up", (4, 16), True, 20, 0),       # UpBlock(in, out): its ResidualBlock is (in + out) -> out
    ("up", (16, 16), False, 32, 0),
    ("downsample", (16,), None, 16, 4),
]
CASES_3D = [
    ("res", (16, 16), None, 16, 0),
    ("down", (16, 16), False, 16, 0),
    ("middle", (16, 16), False, 16, 0),
    ("up", (8, 8), False, 16, 0),
    ("downsample", (16,), None, 16, 2),
]


def _build(kind, args, attn, n_vb, nd, pad):
    from models.enc_proc_dec_components import proc_unet_modern as pu
    torch.manual_seed(0)
    if kind == "downsample":
        m = pu.Downsample(*args, num_spatial_dims=nd, n_cond=n_vb, padding_kwargs=pad)
    elif kind == "res":
        m = pu.ResidualBlock(*args, activation=nn.GELU(), norm=True, num_spatial_dims=nd, padding_kwargs=pad)
    else:
        cls = {"down": pu.DownBlock, "middle": pu.MiddleBlock, "up": pu.UpBlock}[kind]
        m = cls(*args, has_attn=attn, activation=nn.GELU(), norm=True, num_spatial_dims=nd, padding_kwargs=pad)
    return m.to(DEV)


def _inputs(c_x, c_vb, size):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((size[0], c_x) + size[1:], generator=g).to(DEV)
    vb = torch.randn((size[0], c_vb) + size[1:], generator=g).to(DEV) if c_vb else None
    return x, vb


def _forms():
    from models.common import to_ndhwc, to_ncdhw
    from nps_hip import ops, autograd as ad
    # method, source tuple, spatial dims, layout in, layout out
    return {"run": ("run", ops.Src, 2, ops.nchw_to_nhwc, ops.nhwc_to_nchw),
            "run_ad": ("run_ad", ops.Src, 2, ad.to_nhwc, ad.to_nchw),
            "run3d": ("run3d", ops.Src3, 3, to_ndhwc, to_ncdhw)}


def _by_hand(kind, m, x, vb, form):
    """What forward(x, vb) stands for, spelled out on the channels-last entry points."""
    run, Src, nd, to_in, to_out = _forms()[form]
    xh = to_in(x)
    vh = to_in(vb) if vb is not None else None
    if kind == "downsample":
        return tuple(to_out(t) for t in getattr(m, run)(xh, vh))
    srcs = [Src(xh)] + ([Src(vh)] if vh is not None else [])

    def attn(h):
        return h if isinstance(m.attn, nn.Identity) else getattr(m.attn, run)(h)
    if kind == "res":
        y = getattr(m, run)(srcs, xh.shape[1:1 + nd])
    elif kind in ("down", "up"):
        y = attn(getattr(m.res, run)(srcs, xh.shape[1:1 + nd]))
    else:
        h = attn(getattr(m.res1, run)(srcs, xh.shape[1:1 + nd]))
        y = getattr(m.res2, run)([Src(h)], h.shape[1:1 + nd])
    return to_out(y)


def _forward(kind, m, x, vb):
    """forward() as its callers use it -> the tuple of tensors it computes (the pass-through conditioning of a
    Down / MiddleBlock is checked here and dropped)."""
    if kind in ("res", "up"):
        return (m(x),)
    out = m(x, vb)
    if kind == "downsample":
        return tuple(out)
    assert out[1] is vb
    return (out[0],)


def _same(got, want):
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.isfinite(g).all() and torch.equal(g, w)


@pytest.mark.parametrize("pad", PADS, ids=PAD_IDS)
@pytest.mark.parametrize("case", CASES_2D, ids=lambda c: f"{c[0]}{'x'.join(map(str, c[1]))}")
def test_forward_is_the_composition_2d(case, pad):
    kind, args, attn, c_x, c_vb = case
    m = _build(kind, args, attn, c_vb, 2, pad)
    x, vb = _inputs(c_x, c_vb, (2, 12, 10))
    with torch.no_grad():
        _same(_forward(kind, m, x, vb), _by_hand(kind, m, x, vb, "run"))
    got = _forward(kind, m, x, vb)                                    # grad mode, trainable parameters
    assert all(t.requires_grad for t in got)
    _same(got, _by_hand(kind, m, x, vb, "run_ad"))
    sum(t.sum() for t in got).backward()
    for k, p in m.named_parameters():
        if k.startswith("attn.norm."):
            assert p.grad is None, k                                  # AttentionBlock.norm is never applied
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k


@pytest.mark.parametrize("pad", PADS, ids=PAD_IDS)
@pytest.mark.parametrize("case", CASES_3D, ids=lambda c: c[0])
def test_forward_is_the_composition_3d(case, pad):
    kind, args, attn, c_x, c_vb = case
    m = _build(kind, args, attn, c_vb, 3, pad)
    x, vb = _inputs(c_x, c_vb, (1, 6, 6, 8))
    with torch.no_grad():
        _same(_forward(kind, m, x, vb), _by_hand(kind, m, x, vb, "run3d"))


def _unet3d():
    from models.enc_proc_dec_components import UNetModern
    torch.manual_seed(0)
    return UNetModern(pde=None, num_spatial_dims=3, n_cond=2, hidden_features=16, activation=nn.GELU(), norm=True,
                      ch_mults=(1,), is_attn=(False,), n_blocks=1, padding_mode="circular").to(DEV)


def test_unet_forward_is_the_composition_3d():
    from models.common import to_ndhwc, to_ncdhw
    m = _unet3d()
    x, vb = _inputs(16, 2, (1, 6, 6, 8))
    with torch.no_grad():
        _same((m(x, vb),), to_ncdhw(m.run3d(to_ndhwc(x), to_ndhwc(vb))))


@pytest.mark.parametrize("kind", ["unet", "res", "down", "middle"])
def test_3d_refused_under_autograd(kind):
    """Grad mode with trainable parameters: there is no 3-D backward, so no 3-D forward() may hand back a result
    that carries no graph."""
    if kind == "unet":
        m, (x, vb) = _unet3d(), _inputs(16, 2, (1, 6, 6, 8))
    else:
        m, (x, vb) = _build(kind, (16, 16), False, 0, 3, PADS[1]), _inputs(16, 0, (1, 6, 6, 8))
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError):
        m(x) if kind == "res" else m(x, vb)


@pytest.mark.parametrize("padding_mode", PAD_IDS)
def test_unet_inference_and_autograd_forward_agree(padding_mode):
    """Two levels with attention at the lower level and in the middle, conditioning, GroupNorm: the fused inference
    chain and the unfused autograd chain walk the same modules with the same frames.  24x20: the lower level
    is 11x9 in circular mode (valid convs), where conv2 of a ResidualBlock still has a 7x5 output."""
    from models.enc_proc_dec_components import UNetModern
    torch.manual_seed(0)
    m = UNetModern(pde=None, num_spatial_dims=2, n_cond=2, hidden_features=16, activation=nn.GELU(), norm=True,
                   ch_mults=(1, 2), is_attn=(False, True), mid_attn=True, n_blocks=1,
                   padding_mode=padding_mode).to(DEV)
    x, vb = _inputs(16, 2, (2, 24, 20))
    with torch.no_grad():
        y_inf = m(x, vb)
    y_ad = m(x, vb)
    assert y_ad.requires_grad and not y_inf.requires_grad and y_inf.shape == x.shape
    err = rel_l2(y_ad, y_inf)
    print(f"U-Net {padding_mode}: autograd forward vs inference rel-L2 {err:.3e}")
    assert err < TOL
