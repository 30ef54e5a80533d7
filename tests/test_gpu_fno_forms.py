"""The FNO family's forward() against the hand-written composition of its channels-last entry points, at every grid
rank, in the inference and the autograd form (and the 3-D bf16-storage form), bit for bit; and which parameters the
autograd form reaches.

The goldens (tests/test_gpu_parity.py, test_gpu_spectral1d.py, test_gpu_film.py, test_gpu_ufno3d.py, ...) stay the
pin against the reference: this file pins the one module boundary behind these forward()s (models.common.run_flat),
which the compositions below never call, and the one layer / block body per mode behind the entry points.
"""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, K, B = 16, 4, 2  # channels, conditioning channels, batch


# ------------------------------------------------------------------ the flat view, spelled out per rank
def _flat(t):
    """(B, C, *spatial) -> the (B, C, rows, row) tensor the layout kernels transpose."""
    if t.dim() == 3:
        return t.unsqueeze(2)
    if t.dim() == 5:
        return t.reshape(t.shape[0], t.shape[1], t.shape[2] * t.shape[3], t.shape[4])
    return t


def _unflat(y, x):
    """(B, C', rows, row) -> (B, C', *spatial of x)."""
    if x.dim() == 3:
        return y.squeeze(2)
    if x.dim() == 5:
        return y.reshape((y.shape[0], y.shape[1]) + tuple(x.shape[2:]))
    return y


def _in(t, train):
    from nps_hip import ops, autograd as ad
    if t is None:
        return None
    return ad.to_nhwc(_flat(t)) if train else ops.nchw_to_nhwc(_flat(t))


def _out(y, x, train):
    from nps_hip import ops, autograd as ad
    return _unflat(ad.to_nchw(y) if train else ops.nhwc_to_nchw(y), x)


def _in_bf16(t):
    from nps_hip import ops
    return None if t is None else ops.to_bf16(ops.nchw_to_nhwc(ops.to_f32(_flat(t))))


def _out_bf16(y, x):
    from nps_hip import ops
    return _unflat(ops.to_bf16(ops.nhwc_to_nchw(ops.to_f32(y))), x)


def _depth(x):
    return dict(D=x.shape[2]) if x.dim() == 5 else {}


# ------------------------------------------------------------------ modules, inputs, compositions
def _rand(shape, seed=1, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)


def _layer(spatial, modes, conv_mode="single", film=False):
    from models.enc_proc_dec_components.proc_fno import FNO_Layer
    torch.manual_seed(0)
    m = FNO_Layer(hidden_dim=C, num_spatial_dims=len(spatial), modes=modes, conv_mode=conv_mode,
                  feature_transform=film, feature_transform_dim=K).to(DEV)
    return m, dict(x=_rand((B, C) + spatial), p=_rand((B, K), 2) if film else None)


def _layer_fwd(m, x, p):
    return m(x, p) if p is not None else m(x)


def _layer_hand(m, train, x, p):
    from nps_hip import ops
    h = _in(x, train)
    y = m.run_ad(h, p=p, **_depth(x)) if train else m.run([ops.Src(h)], p=p, **_depth(x))
    return _out(y, x, train)


def _fno(spatial, modes, dtype=torch.float32):
    from models.enc_proc_dec_components.proc_fno import FNO
    torch.manual_seed(0)
    m = FNO(pde=None, num_spatial_dims=len(spatial), n_cond=K, hidden_features=C, fno_modes=modes, hidden_blocks=2,
            cond_mode="concat").to(DEV)
    return m, dict(x=_rand((B, C) + spatial, 1, dtype), vb=_rand((B, K) + spatial, 2, dtype))


def _proc_fwd(m, x, vb):
    return m(x, variables_broadcast=vb)


def _fno_hand(m, train, x, vb):
    if x.dtype == torch.bfloat16:
        vh = _in_bf16(vb)
        return _out_bf16(m.run_bf16(_in_bf16(x), vh, x.shape[2]), x)
    vh = _in(vb, train)
    return _out((m.run_ad if train else m.run)(_in(x, train), vh, **_depth(x)), x, train)


def _ufno(spatial, modes, padding_mode, dtype=torch.float32):
    from models.enc_proc_dec_components.proc_ufno import UFNO
    torch.manual_seed(0)
    m = UFNO(pde=None, num_spatial_dims=len(spatial), n_cond=2, hidden_features=C, hidden_blocks=2, fno_modes=modes,
             cond_mode="concat", padding_mode=padding_mode, activation=nn.GELU(), norm=True, ch_mults=(1, 1),
             is_attn=(False, False)).to(DEV)
    return m, dict(x=_rand((B, C) + spatial, 1, dtype), vb=_rand((B, 2) + spatial, 2, dtype))


def _ufno_hand(m, train, x, vb):
    from models.common import to_ndhwc, to_ncdhw, ad_to_ndhwc, ad_to_ncdhw
    if x.dim() != 5:  # the (B, rows, row, C) maps
        vh = _in(vb, train)
        return _out((m.run_ad if train else m.run)(_in(x, train), vh), x, train)
    if train:  # NDHWC volumes
        return ad_to_ncdhw(m.run_ad3d(ad_to_ndhwc(x), ad_to_ndhwc(vb)))
    vh = to_ndhwc(vb)
    return to_ncdhw(m.run3d(to_ndhwc(x), vh))


def _spectral1d():
    from models.enc_proc_dec_components.proc_fno import SpectralConv1d
    torch.manual_seed(0)
    return SpectralConv1d(C, C, (5,)).to(DEV), dict(x=_rand((B, C, 64)))


def _spectral1d_hand(m, train, x):
    from nps_hip import ops, autograd as ad
    if train:
        return ad.to_nchw(m.run_ad(ad.to_nhwc(x.unsqueeze(2)))).squeeze(2)
    y = m.run([ops.Src(ops.nchw_to_nhwc(x.unsqueeze(2)))])  # (B, L, Cout)
    return ops.nhwc_to_nchw(y.unsqueeze(1)).squeeze(2)


def _conv3d():
    from models.common import Conv3d
    torch.manual_seed(0)
    return Conv3d(C, 24, kernel_size=1).to(DEV), dict(x=_rand((B, C, 4, 6, 8)))


def _conv3d_hand(m, train, x):
    from nps_hip import ops, autograd as ad
    Bx, Cx, D, H, W = x.shape
    x4 = x.reshape(Bx, Cx, D * H, W)
    if train:
        y = ad.to_nchw(m.run_ad(ad.to_nhwc(x4)))
    else:
        y = ops.nhwc_to_nchw(m.run([ops.Src(ops.nchw_to_nhwc(x4))], (D * H, W)))
    return y.reshape(Bx, 24, D, H, W)


BF16 = torch.bfloat16
# id -> (build() -> (module, inputs), forward(m, **inputs), by_hand(m, train, **inputs), modes it runs in)
BOTH, INFERENCE = (False, True), (False,)
CASES = {}
for _L in (64, 40):                                     # L = 64 folds into 32-point rows, L = 40 does not
    for _cm in ("single", "double"):
        for _film in (False, True):
            CASES[f"layer1d-L{_L}-{_cm}{'-film' if _film else ''}"] = (
                lambda L=_L, cm=_cm, film=_film: _layer((L,), 5, cm, film), _layer_fwd, _layer_hand, BOTH)
for _cm in ("single", "double"):                        # 12 x 10: the unfused route
    for _film in (False, True):
        CASES[f"layer2d-12x10-{_cm}{'-film' if _film else ''}"] = (
            lambda cm=_cm, film=_film: _layer((12, 10), (4, 4), cm, film), _layer_fwd, _layer_hand, BOTH)
CASES["layer2d-8x128-fused"] = (lambda: _layer((8, 128), (4, 4)), _layer_fwd, _layer_hand, BOTH)  # the spec_z route
CASES["layer3d"] = (lambda: _layer((4, 6, 8), (2, 3, 3)), _layer_fwd, _layer_hand, BOTH)
CASES["fno1d"] = (lambda: _fno((64,), 5), _proc_fwd, _fno_hand, BOTH)
CASES["fno2d"] = (lambda: _fno((12, 10), (4, 4)), _proc_fwd, _fno_hand, BOTH)
CASES["fno3d"] = (lambda: _fno((4, 6, 8), (2, 3, 3)), _proc_fwd, _fno_hand, BOTH)
CASES["fno3d-bf16"] = (lambda: _fno((4, 6, 8), (2, 3, 3), BF16), _proc_fwd, _fno_hand, INFERENCE)
CASES["ufno1d-ones"] = (lambda: _ufno((64,), 5, "ones"), _proc_fwd, _ufno_hand, BOTH)
CASES["ufno2d-circular"] = (lambda: _ufno((16, 16), (4, 4), "circular"), _proc_fwd, _ufno_hand, BOTH)
# 3-D circular convs are valid convs: the second level of ch_mults (1, 1) is (n - 3) // 2 + 1 wide and its
# ResidualBlock needs 5, so 11 per axis is the smallest volume this U-Net runs on (8 leaves conv2 an empty output)
VOL = (11, 12, 13)
CASES["ufno3d-circular"] = (lambda: _ufno(VOL, (2, 3, 3), "circular"), _proc_fwd, _ufno_hand, BOTH)
CASES["ufno3d-circular-bf16"] = (lambda: _ufno(VOL, (2, 3, 3), "circular", BF16), _proc_fwd, _ufno_hand, INFERENCE)
CASES["spectral1d"] = (_spectral1d, lambda m, x: m(x), _spectral1d_hand, BOTH)
CASES["conv3d-pointwise"] = (_conv3d, lambda m, x: m(x), _conv3d_hand, BOTH)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)


def _check_grads(m):
    """Every parameter of these modules is on the route: a finite, non-zero gradient each."""
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        g = torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
        p.grad = None


@pytest.mark.parametrize("name", list(CASES))
def test_forward_is_the_composition(name):
    build, forward, by_hand, modes = CASES[name]
    m, inputs = build()
    if name == "layer2d-8x128-fused":
        from nps_hip import ops
        assert ops.spectral_fusable(128, m.conv.modes2, m.conv.out_channels)
    with torch.no_grad():
        got = forward(m, **inputs)
        assert not got.requires_grad and got.shape[2:] == inputs["x"].shape[2:]
        _same(got, by_hand(m, False, **inputs))
    if True not in modes:
        return
    got = forward(m, **inputs)                            # grad mode, trainable parameters
    assert got.requires_grad
    want = by_hand(m, True, **inputs)
    _same(got, want)
    got.sum().backward()
    _check_grads(m)
    want.sum().backward()
    _check_grads(m)
