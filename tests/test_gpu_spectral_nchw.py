"""GPU parity of the channels-first (NCHW / NCDHW) spectral convolutions: the `_nchw` composites and W-pass stage
entry points of include/nps.h called through ctypes on raw pointers of channels-first device tensors (no layout
change anywhere in this file), ops.spectral_conv2d_nchw and the SpectralConv2d / SpectralConv3d modules' forward.

Yardsticks: the committed goldens and the CPU oracle (oracle.functional.spectral_conv2d / 3d; gradients by torch
autograd through it).  Tolerance: fp32 rel-L2 < 1e-5, the bar of every spectral test.  y and dx are NaN-filled
before each call, so an unwritten element fails the comparison; where an operand is a channel slice of a larger
tensor, the other channels must keep their bits.

Dispatch conditions of the two launchers and the case on each side:
  analysis (dft_w_nchw_kernel)
    bins <= 16 (one pass) / > 16 (passes of 16)        : every other case / (1, 8, 8, 4, 32, 2, 17)
    odd W, W % 32 != 0 (zero-filled chunk tail)        : (2, 5, 3, 6, 7, 4, 3), W = 40
    C % 32 != 0, C > 32 (several tiles, idle waves)    : 5, 36, 132, 196 / 8
    dynamic LDS <= 64 KiB / above (attribute set)      : every other case / W = 600
    W too large for the table                          : refused on the host (tests/test_spectral_nchw_host.py)
  synthesis (idft_w_nchw_kernel<KC, PX>)
    KC = 4 / 8 / 12 / 16 / 16 chunked                  : m2 = 3 / 6 (W = 600) / 9, 10 / 12 (3-D) / 17
    PX = 1 (W <= 64) / PX = 2                          : W = 7, 32, 40, 64 / W = 128, 256, 600
    one pixel tile / several (W > 512)                 : every other case / W = 600
    Cout <= 64 (one staged tile) / more, with a tail   : 3, 8, 44 / 68, 192
    rows per work-group 1 / > 1 with a partial group   : every composite case / the 4500-row stage test
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import functional as Fo
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"


def _lib():
    from nps_hip import lib
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    if rc != 0:
        raise AssertionError(f"{what}: rc {rc}: {_lib().nps_last_error().decode()}")


def _ws(nbytes):
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)


def _bs(t):
    """Batch stride in elements of a channels-first device tensor whose (C, *spatial) block is contiguous."""
    assert t[0].is_contiguous()
    return t.stride(0) if t.shape[0] > 1 else 0


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fwd2d(xd, w1, w2, yd, accumulate=0, act=0):
    """xd (B, Cin, H, W) / yd (B, Cout, H, W): channels-first device tensors, possibly channel slices."""
    lib = _lib()
    B, Cin, H, W = xd.shape
    Cout, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
    w1d, w2d = w1.contiguous().to(DEV), w2.contiguous().to(DEV)
    ws = _ws(lib.nps_spectral_conv2d_workspace(B, Cin, Cout, H, W, m1, m2))
    _ok(lib.nps_spectral_conv2d_fwd_nchw(_p(xd), _bs(xd), _p(w1d), _p(w2d), _p(yd), _bs(yd), _p(ws), B, Cin, Cout, H, W,
                                         m1, m2, accumulate, act, _s()), "spectral_conv2d_fwd_nchw")
    torch.cuda.synchronize()
    return yd


def bwd2d(xd, w1, w2, gd, dxd):
    lib = _lib()
    B, Cin, H, W = xd.shape
    Cout, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
    w1d, w2d = w1.contiguous().to(DEV), w2.contiguous().to(DEV)
    dw1 = torch.full_like(w1d, float("nan"))
    dw2 = torch.full_like(w2d, float("nan"))
    ws = _ws(lib.nps_spectral_conv2d_workspace(B, Cin, Cout, H, W, m1, m2))
    _ok(lib.nps_spectral_conv2d_bwd_nchw(_p(xd), _bs(xd), _p(w1d), _p(w2d), _p(gd), _bs(gd), _p(dxd), _bs(dxd),
                                         _p(dw1), _p(dw2), _p(ws), B, Cin, Cout, H, W, m1, m2, _s()),
        "spectral_conv2d_bwd_nchw")
    torch.cuda.synchronize()
    return dxd, dw1.cpu(), dw2.cpu()


def fwd3d(xd, ws4, yd, accumulate=0, act=0):
    lib = _lib()
    B, Cin, D, H, W = xd.shape
    Cout, m1, m2, m3 = ws4[0].shape[1:]
    wd = [w.contiguous().to(DEV) for w in ws4]
    ws = _ws(lib.nps_spectral_conv3d_workspace(B, Cin, Cout, D, H, W, m1, m2, m3))
    _ok(lib.nps_spectral_conv3d_fwd_nchw(_p(xd), _bs(xd), *[_p(w) for w in wd], _p(yd), _bs(yd), _p(ws), B, Cin, Cout,
                                         D, H, W, m1, m2, m3, accumulate, act, _s()), "spectral_conv3d_fwd_nchw")
    torch.cuda.synchronize()
    return yd


def bwd3d(xd, ws4, gd, dxd):
    lib = _lib()
    B, Cin, D, H, W = xd.shape
    Cout, m1, m2, m3 = ws4[0].shape[1:]
    wd = [w.contiguous().to(DEV) for w in ws4]
    dws = [torch.full_like(w, float("nan")) for w in wd]
    ws = _ws(lib.nps_spectral_conv3d_workspace(B, Cin, Cout, D, H, W, m1, m2, m3))
    _ok(lib.nps_spectral_conv3d_bwd_nchw(_p(xd), _bs(xd), *[_p(w) for w in wd], _p(gd), _bs(gd), _p(dxd), _bs(dxd),
                                         *[_p(d) for d in dws], _p(ws), B, Cin, Cout, D, H, W, m1, m2, m3, _s()),
        "spectral_conv3d_bwd_nchw")
    torch.cuda.synchronize()
    return dxd, [d.cpu() for d in dws]


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", ["spectral2d_a", "spectral2d_overlap", "spectral2d_nyq"])
def test_spectral2d_nchw_golden_forward_backward(name):
    g = load_golden(name)
    w1, w2 = g["state_dict"]["weights1"], g["state_dict"]["weights2"]
    xd = g["x"].contiguous().to(DEV)
    y = fwd2d(xd, w1, w2, _nan(*g["y"].shape))
    assert rel_l2(y.cpu(), g["y"]) < TOL
    dx, dw1, dw2 = bwd2d(xd, w1, w2, g["g"].contiguous().to(DEV), _nan(*g["x"].shape))
    assert rel_l2(dx.cpu(), g["dx"]) < TOL
    assert rel_l2(dw1, g["dw1"]) < TOL
    assert rel_l2(dw2, g["dw2"]) < TOL


@pytest.mark.parametrize("name", ["spectral3d", "spectral3d_overlap", "spectral3d_nyq"])
def test_spectral3d_nchw_golden(name):
    g = load_golden(name)
    ws4 = [g["state_dict"][f"weights{i}"] for i in range(1, 5)]
    xd = g["x"].contiguous().to(DEV)
    assert rel_l2(fwd3d(xd, ws4, _nan(*g["y"].shape)).cpu(), g["y"]) < TOL
    if "g" in g:
        dx, dws = bwd3d(xd, ws4, g["g"].contiguous().to(DEV), _nan(*g["x"].shape))
        assert rel_l2(dx.cpu(), g["dx"]) < TOL
        for i in range(4):
            assert rel_l2(dws[i], g["dw"][i]) < TOL, f"weights{i + 1}"


@pytest.mark.parametrize("want", ["weights", "input"])
def test_spectral2d_nchw_autograd_partial_gradients(want):
    """nps_hip.autograd.spectral_conv2d_nchw with only some gradients requested, on the overlapping-corners fixture:
    weights only (x frozen: no dx), input only (weights frozen: dx and no weight gradient)."""
    from models.enc_proc_dec_components.proc_fno import SpectralConv2d
    from nps_hip import autograd as ad
    g = load_golden("spectral2d_overlap")
    kw = g["kwargs"]
    m = SpectralConv2d(kw["in_channels"], kw["out_channels"], tuple(kw["modes"]))
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV).requires_grad_(want == "weights")
    x = g["x"].to(DEV).requires_grad_(want == "input")
    ad.spectral_conv2d_nchw(m, x).backward(g["g"].to(DEV))
    if want == "weights":
        assert x.grad is None
        assert rel_l2(m.weights1.grad, g["dw1"]) < TOL
        assert rel_l2(m.weights2.grad, g["dw2"]) < TOL
    else:
        assert m.weights1.grad is None and m.weights2.grad is None
        assert rel_l2(x.grad, g["dx"]) < TOL


# ------------------------------------------------------------------ oracle + autograd
@functools.lru_cache(maxsize=None)
def _case2d(B, Cin, Cout, H, W, m1, m2):
    """Inputs, the oracle's output and its autograd gradients, computed once per shape on the CPU."""
    torch.manual_seed(B * 1000 + Cin * 10 + W)
    w1 = (torch.rand(Cin, Cout, m1, m2, dtype=torch.cfloat) / (Cin * Cout)).requires_grad_(True)
    w2 = (torch.rand(Cin, Cout, m1, m2, dtype=torch.cfloat) / (Cin * Cout)).requires_grad_(True)
    x = torch.randn(B, Cin, H, W, requires_grad=True)
    y = Fo.spectral_conv2d(x, w1, w2)
    g = torch.randn_like(y)
    y.backward(g)
    return dict(x=x.detach(), w1=w1.detach(), w2=w2.detach(), y=y.detach(), g=g, dx=x.grad, dw1=w1.grad, dw2=w2.grad)


CASES_2D = [(2, 36, 44, 24, 40, 7, 9), (1, 8, 8, 4, 32, 2, 17), (2, 132, 68, 8, 64, 3, 10),
            (1, 196, 192, 16, 256, 8, 10), (1, 4, 4, 4, 600, 2, 6)]


@pytest.mark.parametrize("shape", CASES_2D, ids=lambda s: "x".join(map(str, s)))
def test_spectral2d_nchw_vs_oracle(shape):
    c = _case2d(*shape)
    xd = c["x"].to(DEV)
    y = fwd2d(xd, c["w1"], c["w2"], _nan(*c["y"].shape))
    assert rel_l2(y.cpu(), c["y"]) < TOL
    dx, dw1, dw2 = bwd2d(xd, c["w1"], c["w2"], c["g"].to(DEV), _nan(*c["x"].shape))
    assert rel_l2(dx.cpu(), c["dx"]) < TOL
    assert rel_l2(dw1, c["dw1"]) < TOL
    assert rel_l2(dw2, c["dw2"]) < TOL


def test_spectral2d_nchw_channel_slices():
    """Odd W, channel counts not multiples of 4, every activation operand a channel slice of a larger tensor: x is
    channels [1:6] of 7 (batch stride 7*H*W, pointer 168 B past a 16-B boundary), y channels [2:5] of a NaN-filled
    6-channel tensor, dy / dx sliced the same way.  The other channels keep their bits."""
    B, Cin, Cout, H, W, m1, m2 = 2, 5, 3, 6, 7, 4, 3
    c = _case2d(B, Cin, Cout, H, W, m1, m2)
    xbig = torch.randn(B, 7, H, W, device=DEV)
    xbig[:, 1:6] = c["x"].to(DEV)
    xs = xbig[:, 1:6]
    assert (xs.data_ptr() - xbig.data_ptr()) == 168 and xs.stride(0) == 7 * H * W
    ybig = _nan(B, 6, H, W)
    y0 = ybig.clone()
    fwd2d(xs, c["w1"], c["w2"], ybig[:, 2:5])
    assert rel_l2(ybig[:, 2:5].cpu(), c["y"]) < TOL
    assert _same_bits(ybig[:, :2], y0[:, :2]) and _same_bits(ybig[:, 5:], y0[:, 5:])
    gbig = torch.randn(B, 6, H, W, device=DEV)
    gbig[:, 2:5] = c["g"].to(DEV)
    dxbig = _nan(B, 7, H, W)
    d0 = dxbig.clone()
    x0 = xbig.clone()
    _, dw1, dw2 = bwd2d(xs, c["w1"], c["w2"], gbig[:, 2:5], dxbig[:, 1:6])
    assert rel_l2(dxbig[:, 1:6].cpu(), c["dx"]) < TOL
    assert _same_bits(dxbig[:, :1], d0[:, :1]) and _same_bits(dxbig[:, 6:], d0[:, 6:])
    assert torch.equal(xbig, x0)
    assert rel_l2(dw1, c["dw1"]) < TOL
    assert rel_l2(dw2, c["dw2"]) < TOL


@pytest.mark.parametrize("shape", [(2, 36, 44, 24, 40, 7, 9), (1, 196, 192, 16, 256, 8, 10)],
                         ids=lambda s: "x".join(map(str, s)))
def test_spectral2d_nchw_accumulate_gelu(shape):
    """FNO_Layer's tail act(y0 + conv(x)) (proc_fno.py:142-146) in the synthesis pass."""
    c = _case2d(*shape)
    torch.manual_seed(11)
    y0 = torch.randn_like(c["y"])
    y = fwd2d(c["x"].to(DEV), c["w1"], c["w2"], y0.to(DEV), accumulate=1, act=1)
    assert rel_l2(y.cpu(), F.gelu(y0 + c["y"])) < TOL


def test_spectral3d_nchw_vs_oracle_forward_backward():
    torch.manual_seed(21)
    B, Cin, Cout, D, H, W, m = 2, 5, 6, 5, 4, 7, (3, 3, 2)
    ws4 = [(torch.rand(Cin, Cout, *m, dtype=torch.cfloat) / (Cin * Cout)).requires_grad_(True) for _ in range(4)]
    x = torch.randn(B, Cin, D, H, W, requires_grad=True)
    ref = Fo.spectral_conv3d(x, *ws4)
    g = torch.randn_like(ref)
    ref.backward(g)
    wd = [w.detach() for w in ws4]
    xd = x.detach().to(DEV)
    assert rel_l2(fwd3d(xd, wd, _nan(*ref.shape)).cpu(), ref.detach()) < TOL
    dx, dws = bwd3d(xd, wd, g.to(DEV), _nan(*x.shape))
    assert rel_l2(dx.cpu(), x.grad) < TOL
    for i in range(4):
        assert rel_l2(dws[i], ws4[i].grad) < TOL, f"weights{i + 1}"


def test_spectral3d_nchw_c5_channels():
    """The C5 channel counts (68 -> 64) and row length (128) on a small volume: forward and accumulate + GELU."""
    torch.manual_seed(22)
    B, Cin, Cout, D, H, W, m = 1, 68, 64, 4, 8, 128, (2, 3, 12)
    ws4 = [torch.rand(Cin, Cout, *m, dtype=torch.cfloat) / (Cin * Cout) for _ in range(4)]
    x = torch.randn(B, Cin, D, H, W)
    ref = Fo.spectral_conv3d(x, *ws4)
    xd = x.to(DEV)
    assert rel_l2(fwd3d(xd, ws4, _nan(*ref.shape)).cpu(), ref) < TOL
    y0 = torch.randn_like(ref)
    assert rel_l2(fwd3d(xd, ws4, y0.to(DEV), accumulate=1, act=1).cpu(), F.gelu(y0 + ref)) < TOL


def test_w_pass_stages_many_rows():
    """The two stage entry points alone on 4500 rows (several rows per synthesis work-group, the last group
    partial) against torch.fft: X1 = rfft(x)[..., :m2] as [B][H][m2][C]; out = irfft(Z, n=W) / H."""
    lib = _lib()
    torch.manual_seed(23)
    B, C, H, W, m2 = 3, 3, 1500, 10, 4
    x = torch.randn(B, C, H, W)
    X1 = torch.full((B, H, m2, C), float("nan"), dtype=torch.complex64, device=DEV)
    xd = x.to(DEV)
    _ok(lib.nps_spectral_dft_w_nchw(_p(xd), 0, B, H, W, C, m2, _p(X1), _s()), "spectral_dft_w_nchw")
    ref = torch.einsum("bchk->bhkc", torch.fft.rfft(x, dim=-1)[..., :m2])
    assert rel_l2(torch.view_as_real(X1.cpu()), torch.view_as_real(ref.contiguous())) < TOL
    Z = torch.randn(B, H, m2, C, dtype=torch.complex64)
    out = _nan(B, C, H, W)
    Zd = Z.to(DEV)
    _ok(lib.nps_spectral_idft_w_nchw(_p(Zd), _p(out), 0, B, H, W, m2, C, 0, 0, _s()), "spectral_idft_w_nchw")
    torch.cuda.synchronize()
    Zf = torch.zeros(B, C, H, W // 2 + 1, dtype=torch.complex64)
    Zf[..., :m2] = torch.einsum("bhkc->bchk", Z)
    assert rel_l2(out.cpu(), torch.fft.irfft(Zf, n=W, dim=-1) / H) < TOL


# ------------------------------------------------------------------ Python layer
def test_ops_spectral_conv2d_nchw_batch_strided_view():
    from nps_hip import ops
    B, Cin, Cout, H, W, m1, m2 = 2, 5, 3, 6, 7, 4, 3
    c = _case2d(B, Cin, Cout, H, W, m1, m2)
    xbig = torch.randn(B, 7, H, W, device=DEV)
    xbig[:, 1:6] = c["x"].to(DEV)
    wp = ops.pack_spectral_weight(c["w1"].to(DEV), c["w2"].to(DEV), H)
    y = ops.spectral_conv2d_nchw(xbig[:, 1:6], wp, m1, m2, Cout)
    assert y.shape == (B, Cout, H, W) and rel_l2(y, c["y"]) < TOL
    ybig = _nan(B, 6, H, W)
    ops.spectral_conv2d_nchw(xbig[:, 1:6], wp, m1, m2, Cout, out=ybig[:, 2:5])
    assert rel_l2(ybig[:, 2:5], c["y"]) < TOL and bool(torch.isnan(ybig[:, :2]).all())


def _no_transposes(monkeypatch):
    from nps_hip import ops

    def boom(*a, **k):
        raise AssertionError("the module transposed its activations")
    monkeypatch.setattr(ops, "nchw_to_nhwc", boom)
    monkeypatch.setattr(ops, "nhwc_to_nchw", boom)


def test_spectral_conv2d_module_runs_channels_first(monkeypatch):
    from models.enc_proc_dec_components.proc_fno import SpectralConv2d
    c = _case2d(2, 36, 44, 24, 40, 7, 9)
    m = SpectralConv2d(36, 44, (7, 9))
    m.load_state_dict({"weights1": c["w1"], "weights2": c["w2"]})
    m = m.to(DEV)
    _no_transposes(monkeypatch)
    with torch.no_grad():
        assert rel_l2(m(c["x"].to(DEV)), c["y"]) < TOL
    xd = c["x"].to(DEV).requires_grad_(True)
    y = m(xd)
    y.backward(c["g"].to(DEV))
    assert rel_l2(y, c["y"]) < TOL
    assert rel_l2(xd.grad, c["dx"]) < TOL
    assert rel_l2(m.weights1.grad, c["dw1"]) < TOL
    assert rel_l2(m.weights2.grad, c["dw2"]) < TOL


def test_spectral_conv3d_module_runs_channels_first(monkeypatch):
    from models.enc_proc_dec_components.proc_fno import SpectralConv3d
    torch.manual_seed(31)
    m = SpectralConv3d(5, 6, (3, 3, 2))
    x = torch.randn(2, 5, 5, 4, 7)
    ws4 = [getattr(m, f"weights{i}").detach().clone().requires_grad_(True) for i in range(1, 5)]
    xr = x.clone().requires_grad_(True)
    ref = Fo.spectral_conv3d(xr, *ws4)
    g = torch.randn_like(ref)
    ref.backward(g)
    m = m.to(DEV)
    _no_transposes(monkeypatch)
    with torch.no_grad():
        assert rel_l2(m(x.to(DEV)), ref.detach()) < TOL
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    y.backward(g.to(DEV))
    assert rel_l2(y, ref.detach()) < TOL
    assert rel_l2(xd.grad, xr.grad) < TOL
    for i in range(4):
        assert rel_l2(getattr(m, f"weights{i + 1}").grad, ws4[i].grad) < TOL, f"weights{i + 1}"
