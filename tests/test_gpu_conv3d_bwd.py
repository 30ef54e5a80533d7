"""3-D conv backward (csrc/conv3d_bwd.hip, nps_hip.autograd Conv3dFn / ConvTranspose3dFn, models.common Conv3d /
ConvTranspose3d_padded forward under autograd) against torch CPU fp64 autograd of F.conv3d / F.conv_transpose3d
(F.pad(mode="circular") where needed) under a random cotangent, loss = (y * g).sum().  rel-L2 < 1e-5 for each of
y, dx, dw, db: the project's fp32 bar (tests/test_gpu_backward.py, tests/test_gpu_conv3d.py) — storage, MFMA
operands and accumulation are fp32 throughout."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.float32)


def _ncdhw(t):
    return t.detach().cpu().permute(0, 4, 1, 2, 3).double()


def _ref_fwd(kind, x, w, b, stride, mode, p):
    if kind == "convT":
        return F.conv_transpose3d(F.pad(x, (p,) * 6, mode="circular") if p else x, w, b, stride=2)
    if mode == "circular":
        return F.conv3d(F.pad(x, (p,) * 6, mode="circular"), w, b, stride=stride)
    return F.conv3d(x, w, b, stride=stride, padding=p)


@functools.lru_cache(maxsize=None)
def _case(kind, B, Cin, Cout, dhw, K, stride, mode, p, seed=0):
    """Random fp32-representable operands and the fp64 reference (y, dx, dw, db), computed once per geometry."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, *dhw, generator=g)
    wshape = (Cin, Cout, 4, 4, 4) if kind == "convT" else (Cout, Cin, K, K, K)
    w = torch.randn(wshape, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = _ref_fwd(kind, xd, wd, bd, stride, mode, p)
    gy = torch.randn(y.shape, generator=g)
    (y * gy.double()).sum().backward()
    return x, w, b, gy, (y.detach(), xd.grad, wd.grad, bd.grad)


class _Geo:
    """Stands in for the module in ad.conv3d / ad.conv_transpose3d: geometry + parameters."""


def _run_fn(kind, x, w, b, gy, K, stride, mode, p, x_grad=True, w_grad=True, b_grad=True):
    from nps_hip import autograd as ad
    xh = _ndhwc(x).requires_grad_(x_grad)
    wp = nn.Parameter(w.to(DEV), requires_grad=w_grad)
    bp = nn.Parameter(b.to(DEV), requires_grad=b_grad)
    if kind == "convT":
        y = ad.ConvTranspose3dFn.apply((p,), xh, wp, bp)
    else:
        geo = (K, stride, p, 0) if mode == "circular" else (K, stride, 0, p)
        y = ad.Conv3dFn.apply(geo, xh, wp, bp)
    (y * _ndhwc(gy)).sum().backward()
    return y, xh, wp, bp


def _check(kind, B, Cin, Cout, dhw, K=3, stride=1, mode="zeros", p=0):
    x, w, b, gy, (ry, rdx, rdw, rdb) = _case(kind, B, Cin, Cout, dhw, K, stride, mode, p)
    y, xh, wp, bp = _run_fn(kind, x, w, b, gy, K, stride, mode, p)
    errs = dict(y=rel_l2(_ncdhw(y), ry), dx=rel_l2(_ncdhw(xh.grad), rdx), dw=rel_l2(wp.grad, rdw),
                db=rel_l2(bp.grad, rdb))
    print(f"{kind} Cin={Cin} Cout={Cout} {dhw} K={K} s={stride} {mode} p={p}: " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    return xh.grad


# Cin = 20: one 16-channel chunk + a tail of 4, Cout = 40 below one 64 tile, W = 34 crosses the 32-column tile;
# Cin = 68 / Cout = 72 both cross a 64-channel tile (the C5 64 + 4 channel count)
@pytest.mark.parametrize("mode,p", [("zeros", 0), ("zeros", 1), ("circular", 1)], ids=["valid", "zero1", "circ1"])
@pytest.mark.parametrize("Cin,Cout,dhw", [(20, 40, (5, 7, 34)), (68, 72, (4, 6, 10))], ids=["c20x40", "c68x72"])
def test_conv3d_stride1(Cin, Cout, dhw, mode, p):
    _check("conv", 2, Cin, Cout, dhw, mode=mode, p=p)


@pytest.mark.parametrize("p", [0, 1], ids=["valid", "zero1"])
def test_conv3d_stride2(p):
    dx = _check("conv", 2, 20, 24, (6, 7, 9), stride=2, p=p)
    if p == 0:  # depth index 5 is read by no output ((6 - 3) odd): stored, and exactly zero
        assert (dx[:, 5] == 0).all()


@pytest.mark.parametrize("dhw", [(2, 4, 5), (3, 5, 33)], ids=["2x4x5", "3x5x33"])
def test_conv_transpose3d(dhw):
    _check("convT", 2, 24, 20, dhw, p=1)


def test_split_reduction():
    """The forward test's shape: 210 voxel tiles per (m tile, n tile, kd plane) split over 27 work-groups that add
    their partials into dw atomically (nps_conv3d_wgrad_splits, the launcher's own plan)."""
    from nps_hip import ops
    a = torch.empty(2, 7, 18, 38, 48, device=DEV)
    x = torch.empty(2, 9, 20, 40, 68, device=DEV)
    assert ops.conv3d_wgrad_splits(a, x, 3) > 1
    _check("conv", 2, 68, 48, (9, 20, 40))


# ---------------------------------------------------------------- nps_conv3d_wgrad directly
def _wgrad_ref(a, x, K, S, circ, zpad):
    """g[m][n][kd][kh][kw] = sum a[b, m, p] * Xext[b, n, p*S + k] in fp64 (NCDHW inputs)."""
    xe = F.pad(x.double(), (circ,) * 6, mode="circular") if circ else x.double()
    xe = F.pad(xe, (zpad,) * 6)
    a = a.double()
    Da, Ha, Wa = a.shape[2:]
    g = torch.empty(a.shape[1], x.shape[1], K, K, K, dtype=torch.float64)
    for kd in range(K):
        for kh in range(K):
            for kw in range(K):
                xs = xe[:, :, kd:kd + S * (Da - 1) + 1:S, kh:kh + S * (Ha - 1) + 1:S, kw:kw + S * (Wa - 1) + 1:S]
                g[:, :, kd, kh, kw] = torch.einsum("bmdhw,bndhw->mn", a, xs)
    return g


@pytest.mark.parametrize("K,S,circ,zpad,a_dhw,x_dhw,M,N", [
    (4, 2, 1, 0, (4, 6, 18), (8, 12, 36), 24, 20),    # the Upsample's roles and tap grouping, circular x
    (4, 2, 0, 0, (4, 6, 7), (10, 14, 16), 24, 20),    # the Upsample: a = padded input, x = dy
    (2, 1, 0, 0, (4, 6, 18), (5, 7, 19), 36, 70),
    (3, 1, 1, 1, (7, 9, 22), (5, 7, 20), 20, 8),      # circular then zero extension together
    (1, 2, 0, 0, (3, 4, 9), (5, 7, 17), 66, 3),
], ids=["k4s2circ", "k4s2", "k2", "k3circzpad", "k1s2"])
def test_wgrad_direct(K, S, circ, zpad, a_dhw, x_dhw, M, N):
    """ops.conv3d_wgrad on its own, including g pre-filled with a constant: the launch adds to g."""
    from nps_hip import ops
    g = torch.Generator().manual_seed(3)
    a = torch.randn(2, M, *a_dhw, generator=g)
    x = torch.randn(2, N, *x_dhw, generator=g)
    ref = _wgrad_ref(a, x, K, S, circ, zpad)
    got = ops.conv3d_wgrad(_ndhwc(a), _ndhwc(x), K, stride=S, circ=circ, zpad=zpad)
    assert got.shape == ref.shape
    e0 = rel_l2(got, ref)
    pre = torch.full(ref.shape, 0.5, device=DEV)
    out = ops.conv3d_wgrad(_ndhwc(a), _ndhwc(x), K, stride=S, circ=circ, zpad=zpad, g=pre)
    assert out is pre
    e1 = rel_l2(pre, ref + 0.5)
    print(f"wgrad K={K} S={S} circ={circ} zpad={zpad}: {e0:.2e}, += {e1:.2e}")
    assert e0 < TOL and e1 < TOL


def test_layout_helpers():
    """space_to_depth3d, circular_pad3d and circular_fold3d against torch indexing (exact: copies and short sums)."""
    from nps_hip import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 8, 10, 5, generator=g)
    xd = x.to(DEV)
    q = ops.space_to_depth3d(xd, 4, 4, 6).cpu()          # one voxel past x on D and W: zeros
    xz = F.pad(x, (0, 0, 0, 2, 0, 0, 0, 2))              # (2, 8, 8, 12, 5)
    want = xz.reshape(2, 4, 2, 4, 2, 6, 2, 5).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(2, 4, 4, 6, 40)
    assert torch.equal(q, want)
    xc = x.permute(0, 4, 1, 2, 3)
    padded = F.pad(xc, (2,) * 6, mode="circular").permute(0, 2, 3, 4, 1)
    assert torch.equal(ops.circular_pad3d(xd, 2).cpu(), padded)
    gp = torch.randn(2, 10, 12, 14, 5, generator=g)
    xr = xc.double().clone().requires_grad_(True)
    F.pad(xr, (2,) * 6, mode="circular").backward(gp.permute(0, 4, 1, 2, 3).double())
    assert rel_l2(ops.circular_fold3d(gp.to(DEV), 2).permute(0, 4, 1, 2, 3), xr.grad) < 1e-6


# ---------------------------------------------------------------- autograd plumbing
PLUMB = ("conv", 2, 20, 40, (5, 7, 34), 3, 1, "circular", 1)


def test_no_input_gradient():
    x, w, b, gy, (_, _, rdw, rdb) = _case(*PLUMB)
    _, xh, wp, bp = _run_fn("conv", x, w, b, gy, 3, 1, "circular", 1, x_grad=False)
    assert xh.grad is None
    assert rel_l2(wp.grad, rdw) < TOL and rel_l2(bp.grad, rdb) < TOL


def test_frozen_weight_trainable_bias():
    x, w, b, gy, (_, rdx, _, rdb) = _case(*PLUMB)
    _, xh, wp, bp = _run_fn("conv", x, w, b, gy, 3, 1, "circular", 1, w_grad=False)
    assert wp.grad is None
    assert rel_l2(bp.grad, rdb) < TOL and rel_l2(_ncdhw(xh.grad), rdx) < TOL


@pytest.mark.parametrize("kind", ["conv", "convT"])
def test_two_backward_passes_accumulate(kind):
    from nps_hip import autograd as ad
    case = PLUMB if kind == "conv" else ("convT", 2, 24, 20, (2, 4, 5), 3, 1, "zeros", 1)  # (test_conv_transpose3d's case)
    x, w, b, gy, _ = _case(*case)
    xh = _ndhwc(x).requires_grad_(True)
    wp, bp = nn.Parameter(w.to(DEV)), nn.Parameter(b.to(DEV))
    gh = _ndhwc(gy)
    single = None
    for _ in range(2):
        y = ad.ConvTranspose3dFn.apply((1,), xh, wp, bp) if kind == "convT" else ad.Conv3dFn.apply((3, 1, 1, 0), xh, wp, bp)
        (y * gh).sum().backward()
        if single is None:
            single = [t.grad.clone() for t in (xh, wp, bp)]
    for t, s in zip((xh, wp, bp), single):
        assert rel_l2(t.grad, 2 * s) < 1e-6


# ---------------------------------------------------------------- module level (NCDHW, grad mode)
def _module_check(m, conv, kind, x, stride, mode, p):
    """m(x) under grad mode against the fp64 reference with conv's parameters: y, x.grad, every parameter's grad."""
    xd = x.double().requires_grad_(True)
    wd, bd = (t.detach().cpu().double().requires_grad_(True) for t in (conv.weight, conv.bias))
    ry = _ref_fwd(kind, xd, wd, bd, stride, mode, p)
    gy = torch.randn(ry.shape, generator=torch.Generator().manual_seed(7))
    (ry * gy.double()).sum().backward()
    xg = x.to(DEV).requires_grad_(True)
    y = m(xg)
    assert y.requires_grad and y.shape == ry.shape
    (y * gy.to(DEV)).sum().backward()
    assert [k for k, _ in m.named_parameters()] in (["weight", "bias"], ["conv.weight", "conv.bias"])
    errs = dict(y=rel_l2(y, ry), dx=rel_l2(xg.grad, xd.grad), dw=rel_l2(conv.weight.grad, wd.grad),
                db=rel_l2(conv.bias.grad, bd.grad))
    print(type(m).__name__, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs


def _modules():
    from models.common import Conv3d
    from models.enc_proc_dec_components.proc_unet_modern import Downsample, Upsample
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(5)
    conv = Conv3d(20, 40, 3, padding_mode="circular").to(DEV)
    up = Upsample(24, 3, dict(padding_mode="circular")).to(DEV)
    down = Downsample(20, 3, 0, dict(padding_mode="circular")).to(DEV)
    return [(conv, conv, "conv", torch.randn(2, 20, 5, 7, 34, generator=g), 1, "zeros", 0),
            (up, up.conv, "convT", torch.randn(2, 24, 2, 4, 5, generator=g), 2, "circular", 1),
            (down, down.conv, "conv", torch.randn(2, 20, 6, 7, 9, generator=g), 2, "zeros", 0)]


@pytest.mark.parametrize("i", [0, 1, 2], ids=["Conv3d", "Upsample", "Downsample"])
def test_module_forward_is_differentiable(i):
    """Conv3d(20, 40, 3, padding_mode="circular") (padding 0: valid), Upsample and Downsample (n_cond = 0) in 3-D:
    NotImplementedError before this backward existed."""
    _module_check(*_modules()[i])


@pytest.mark.parametrize("i", [0, 1, 2], ids=["Conv3d", "Upsample", "Downsample"])
def test_module_refusals_and_unchanged_inference(i):
    from models.common import to_ncdhw, to_ndhwc
    from nps_hip import ops
    m, conv, kind, x, *_ = _modules()[i]
    x = x.to(DEV)
    with pytest.raises(NotImplementedError):
        m(x.bfloat16())                                            # grad mode, trainable parameters, bf16 input
    with torch.no_grad():
        y = m(x)
        xh = to_ndhwc(x)
        want = conv.run3d(xh) if kind == "convT" else conv.run3d([ops.Src3(xh)], xh.shape[1:4])
        assert not y.requires_grad and torch.equal(y, to_ncdhw(want))
    for p in m.parameters():
        p.requires_grad_(False)
    assert torch.equal(m(x), y)                                    # frozen parameters: the inference path


def test_fn_refuses_bf16_and_unsupported_geometries():
    from nps_hip import autograd as ad
    x = torch.zeros(1, 4, 4, 4, 16, device=DEV)
    w = nn.Parameter(torch.zeros(16, 16, 3, 3, 3, device=DEV))
    with pytest.raises(NotImplementedError, match="fp32 for training"):
        ad.Conv3dFn.apply((3, 1, 0, 0), x.bfloat16(), w, None)
    with pytest.raises(NotImplementedError, match="fp32 for training"):
        ad.ConvTranspose3dFn.apply((1,), x.bfloat16(), nn.Parameter(torch.zeros(16, 16, 4, 4, 4, device=DEV)), None)
    with pytest.raises(NotImplementedError):
        ad.Conv3dFn.apply((3, 2, 1, 0), x, w, None)                # stride 2 with circular padding
