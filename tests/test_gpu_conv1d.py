"""The 1-D conv kernels (csrc/conv1d.hip: nps_conv1d_fwd, nps_conv1d_wgrad; nps_hip.autograd Conv1dFn /
ConvTranspose1dFn; models.common Conv1d / ConvTranspose1d) against the fp64 restatement tests/conv1d_ref.py and
against the nn modules in float64 on the CPU.  Inputs uniform in [-1, 1]; rel-L2 < 1e-5, the bound
tests/test_gpu_conv3d_bwd.py holds the same exact-fp32 MFMA class to.  Shapes: B = 2 (a tap must not read the
neighbouring sample of the flattened B*L axis); L 1 (one point), 7 (odd, a stride-2 tail), 33 (one 32-point tile row
plus one), 64 (exact tiles) and 130 (a third tile of the 64-position work-group tile); channels (2, 2), (18, 16) (a
channel tail past one 16-channel chunk), (34, 40) (three chunks, a Cout tail past one 32-wide MFMA tile) and
(70, 70) (a second 64-channel work-group tile in both gradients)."""
import functools

import pytest
import torch
from torch import nn

import conv1d_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5

LS = [1, 7, 33, 64]
CHANNELS = [(2, 2), (18, 16), (34, 40)]
# (K, stride, (pad_l, pad_r), out_os): the 2-tap phases of the transposed conv run with out_os = 2, both phases
GEOS = [(1, 1, (0, 0), 1), (3, 1, (1, 1), 1), (3, 2, (1, 1), 1), (2, 1, (1, 1), 2), (4, 2, (1, 1), 1)]


def _valid(L, K, s, pad):
    return L + pad[0] + pad[1] >= K


def _dev(t):
    return t.to(DEV).contiguous()


def _fill(shape, seed):
    """what a launch must leave alone: a recognisable fp32 pattern"""
    return R.rand(shape, seed) * 3 + 7


def _check_out(got, ref, before, rows, Cout, what):
    """rel-L2 on the written range, bit-identity with `before` outside it"""
    got = got.cpu()
    mask = torch.zeros(got.shape, dtype=torch.bool)
    mask[:, rows, :Cout] = True
    err = rel_l2(got[mask], ref[mask])
    print(f"{what}: rel-L2 {err:.2e}")
    assert err < TOL, (what, err)
    assert torch.equal(got[~mask], before[~mask]), f"{what}: wrote outside its range"


@pytest.mark.parametrize("L,Cin,Cout,K,s,pad,out_os", [(L, *c, *g) for L in LS for c in CHANNELS for g in GEOS
                                                       if _valid(L, *g[:3])])
def test_forward(L, Cin, Cout, K, s, pad, out_os):
    from nps_hip import ops
    x, w, b = R.rand((2, L, Cin), 1), R.rand((Cout, Cin, K), 2), R.rand((Cout,), 3)
    Lout = R.out_len(L, K, s, pad)
    pk = ops.pack_conv1d_weight(_dev(w))
    if out_os == 1:
        y = ops.conv1d([ops.Src1(_dev(x))], L, pk, _dev(b), Cout, K, stride=s, pad=pad)
        assert tuple(y.shape) == (2, Lout, Cout)
        err = rel_l2(y, R.conv1d_fwd([(x, 0)], L, w, b, stride=s, pad=pad))
        print(f"fwd L={L} C={Cin}->{Cout} K={K} s={s}: rel-L2 {err:.2e}")
        assert err < TOL
        # the same launch into a pre-filled out that is wider (Cout + 3 channels) and longer (2 rows in front, 3
        # behind) than the result: rows past the L tail of the last tile, the next sample's rows and the channels
        # past Cout keep their bits
        before = _fill((2, Lout + 5, Cout + 3), 4)
        out = _dev(before)
        ops.conv1d([ops.Src1(_dev(x))], L, pk, _dev(b), Cout, K, stride=s, pad=pad, out=out, out_off=2)
        ref = R.conv1d_fwd([(x, 0)], L, w, b, stride=s, pad=pad, out=before, out_off=2)
        _check_out(out, ref, before, R.written_rows(Lout, Lout + 5, 1, 2), Cout, f"into out L={L} C={Cin}->{Cout} K={K} s={s}")
        return
    for phase, off in ((0, -1), (1, 0)):  # the transposed conv's phases at padding 1: rows 2 q + phase - 1
        out_L = 2 * L
        before = _fill((2, out_L, Cout + 3), 4)
        out = _dev(before)
        ops.conv1d([ops.Src1(_dev(x))], L, pk, _dev(b), Cout, K, pad=pad, out=out, out_os=2, out_off=off)
        ref = R.conv1d_fwd([(x, 0)], L, w, b, pad=pad, out=before, out_os=2, out_off=off)
        _check_out(out, ref, before, R.written_rows(Lout, out_L, 2, off), Cout, f"phase {phase} L={L} C={Cin}->{Cout}")


@pytest.mark.parametrize("L", [7, 33, 130])
def test_forward_three_source_frame(L):
    """cat((h, crop(skip), crop(vb))): 16 + 16 + 2 channels, the skip one longer and placed at -1, the conditioning
    shorter than the frame and placed at 1; accumulated at offset 2 into a pre-filled out with an addend and GELU"""
    from nps_hip import ops
    h, skip, vb = R.rand((2, L, 16), 1), R.rand((2, L + 1, 16), 2), R.rand((2, max(L - 3, 1), 2), 3)
    w, b = R.rand((40, 34, 3), 4), R.rand((40,), 5)
    srcs = [(h, 0), (skip, -1), (vb, 1)]
    dsrcs = [ops.Src1(_dev(t), o) for t, o in srcs]
    pk = ops.pack_conv1d_weight(_dev(w))
    y = ops.conv1d(dsrcs, L, pk, _dev(b), 40, 3, pad=(1, 1))
    err = rel_l2(y, R.conv1d_fwd(srcs, L, w, b, pad=(1, 1)))
    print(f"three sources L={L}: rel-L2 {err:.2e}")
    assert err < TOL
    before, add = _fill((2, L + 3, 40), 6), R.rand((2, L + 3, 40), 7)
    out = _dev(before)
    ops.conv1d(dsrcs, L, pk, _dev(b), 40, 3, pad=(1, 1), out=out, out_off=2, accumulate=True, addend=_dev(add), act=1)
    ref = R.conv1d_fwd(srcs, L, w, b, pad=(1, 1), out=before, out_off=2, accumulate=True, addend=add, act=1)
    _check_out(out, ref, before, R.written_rows(L, L + 3, 1, 2), 40, f"accumulate + addend + GELU L={L}")
    # the rows of a negative offset that fall outside out are dropped, not wrapped into the neighbouring sample
    before = _fill((2, L, 40), 8)
    out = _dev(before)
    ops.conv1d(dsrcs, L, pk, _dev(b), 40, 3, pad=(1, 1), out=out, out_off=-2, addend=_dev(add[:, :L].contiguous()), act=1)
    ref = R.conv1d_fwd(srcs, L, w, b, pad=(1, 1), out=before, out_off=-2, addend=add[:, :L], act=1)
    _check_out(out, ref, before, R.written_rows(L, L, 1, -2), 40, f"offset -2 L={L}")


@functools.lru_cache(maxsize=None)
def _grad_case(kind, L, Cin, Cout, K, s, p):
    x = R.rand((2, L, Cin), 1)
    w = R.rand((Cin, Cout, 4) if kind == "convT" else (Cout, Cin, K), 2)
    b = R.rand((Cout,), 3)
    if kind == "convT":
        y = R.conv_transpose1d(x, w, b, p)
        gy = R.rand(tuple(y.shape), 4)
        dx = R.conv1d_fwd([(gy, 0)], gy.shape[1], w, None, stride=2, pad=(p, p))
        dw = R.conv1d_dw(x, gy, 4, 2, (p, p))
    else:
        y = R.conv1d_fwd([(x, 0)], L, w, b, stride=s, pad=(p, p))
        gy = R.rand(tuple(y.shape), 4)
        dx = R.conv1d_dx(gy, w, L, s, (p, p))
        dw = R.conv1d_dw(gy, x, K, s, (p, p))
    return x, w, b, gy, (y, dx, dw, gy.double().sum((0, 1)))


def _run_fn(kind, x, w, b, gy, K, s, p):
    from nps_hip import autograd as ad
    xh = _dev(x).unsqueeze(1).requires_grad_(True)
    wp, bp = nn.Parameter(_dev(w)), nn.Parameter(_dev(b))
    y = ad.ConvTranspose1dFn.apply(p, xh, wp, bp) if kind == "convT" else ad.Conv1dFn.apply((K, s, p, p), xh, wp, bp)
    (y * _dev(gy).unsqueeze(1)).sum().backward()
    return y, xh, wp, bp


GRAD_KINDS = [("conv", 1, 1, 0), ("conv", 3, 1, 1), ("conv", 3, 2, 1), ("conv", 4, 2, 1), ("convT", 4, 2, 1),
              ("convT", 4, 2, 0)]
# every length with the three channel pairs; the second 64-channel tile at two lengths
GRAD_SHAPES = [(L, *c) for L in LS + [130] for c in CHANNELS] + [(33, 70, 70), (130, 70, 70)]


@pytest.mark.parametrize("L,Cin,Cout,kind,K,s,p", [(*sh, *k) for sh in GRAD_SHAPES for k in GRAD_KINDS
                                                   if k[0] == "convT" or _valid(sh[0], k[1], k[2], (k[3], k[3]))])
def test_gradients(L, Cin, Cout, kind, K, s, p):
    """y, dx, dw, db of the autograd functions under loss = (y * g).sum() against the restatement"""
    x, w, b, gy, ref = _grad_case(kind, L, Cin, Cout, K, s, p)
    y, xh, wp, bp = _run_fn(kind, x, w, b, gy, K, s, p)
    errs = [rel_l2(g.squeeze(1) if g.dim() == 4 else g, r) for g, r in zip((y, xh.grad, wp.grad, bp.grad), ref)]
    print(f"{kind} L={L} C={Cin}->{Cout} K={K} s={s} p={p}: y {errs[0]:.2e} dx {errs[1]:.2e} dw {errs[2]:.2e} "
          f"db {errs[3]:.2e}")
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("B,L,M,N,K,s", [(2, 33, 34, 40, 3, 1), (16, 600, 18, 16, 3, 2), (2, 130, 70, 70, 4, 2)])
def test_weight_gradient_is_deterministic(B, L, M, N, K, s):
    """the split reduction has a fixed schedule and no atomics: two runs give identical bits (the second shape runs
    more than one split)"""
    from nps_hip import ops
    x = _dev(R.rand((B, L, N), 1))
    a = _dev(R.rand((B, R.out_len(L, K, s, (1, 1)), M), 2))
    g1 = ops.conv1d_wgrad(a, x, K, stride=s, pad=(1, 1))
    junk = torch.full((1 << 20,), 3.0, device=DEV)  # (the second run's workspace need not be the first's memory)
    g2 = ops.conv1d_wgrad(a, x, K, stride=s, pad=(1, 1))
    assert torch.equal(g1, g2) and junk[0] == 3.0
    err = rel_l2(g1, R.conv1d_dw(a.cpu(), x.cpu(), K, s, (1, 1)))
    print(f"wgrad B={B} L={L} {M}x{N} K={K} s={s}: rel-L2 {err:.2e}")
    assert err < TOL


def test_non_fp32_is_refused():
    from nps_hip import ops
    x = torch.zeros(1, 8, 4, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32"):
        ops.pack_conv1d_weight(torch.zeros(4, 4, 3, device=DEV, dtype=torch.bfloat16))
    pk = ops.pack_conv1d_weight(torch.zeros(4, 4, 3, device=DEV))
    with pytest.raises(NotImplementedError, match="fp32"):
        ops.conv1d([ops.Src1(x)], 8, pk, None, 4, 3, pad=(1, 1))
    with pytest.raises(NotImplementedError, match="fp32"):
        ops.conv1d_wgrad(x, x, 3, pad=(1, 1))


def test_short_bias_is_refused():
    from nps_hip import ops
    x = torch.zeros(1, 8, 4, device=DEV)
    pk = ops.pack_conv1d_weight(torch.zeros(4, 4, 3, device=DEV))
    with pytest.raises(RuntimeError, match="bias must hold Cout = 4"):
        ops.conv1d([ops.Src1(x)], 8, pk, torch.zeros(3, device=DEV), 4, 3, pad=(1, 1))


# ------------------------------------------------------------------ modules
def _module_case(make, L, seed=0):
    torch.manual_seed(seed)
    ref = make(nn.Conv1d, nn.ConvTranspose1d).double()
    x = R.rand((2, ref.in_channels, L), 5)
    xd = x.double().requires_grad_(True)
    y = ref(xd)
    gy = R.rand(tuple(y.shape), 6)
    (y * gy.double()).sum().backward()
    return ref, x, gy, (y.detach(), xd.grad, ref.weight.grad, ref.bias.grad)


@pytest.mark.parametrize("name,make", [
    ("conv k3 p1", lambda C, T: C(18, 16, 3, padding=1)),
    ("conv k3 s2 p1", lambda C, T: C(16, 16, 3, stride=2, padding=1)),
    ("convT k4 s2 p1", lambda C, T: T(16, 16, 4, stride=2, padding=1)),
])
@pytest.mark.parametrize("L", [13, 64])
def test_modules_against_nn_in_float64(name, make, L):
    """run (inference) and run_ad (loss = (y * g).sum()) of the models.common modules on (B, 1, L, C) maps against
    the same nn module in float64 on the CPU: output, x gradient, weight and bias gradients"""
    from models import common
    from nps_hip import ops
    ref, x, gy, (ry, rdx, rdw, rdb) = _module_case(make, L)
    m = make(common.Conv1d, common.ConvTranspose1d)
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    m = m.to(DEV)
    cl = lambda t: _dev(t.transpose(1, 2)).unsqueeze(1)          # noqa: E731  (B, C, L) -> (B, 1, L, C)
    back = lambda t: t.squeeze(1).transpose(1, 2)                # noqa: E731
    with torch.no_grad():
        y0 = m.run(cl(x)) if isinstance(m, nn.ConvTranspose1d) else m.run([ops.Src(cl(x))], (1, L))
    xh = cl(x).requires_grad_(True)
    y = m.run_ad(xh)
    (y * cl(gy)).sum().backward()
    errs = dict(run=rel_l2(back(y0), ry), run_ad=rel_l2(back(y), ry), dx=rel_l2(back(xh.grad), rdx),
                dw=rel_l2(m.weight.grad, rdw), db=rel_l2(m.bias.grad, rdb))
    print(f"{name} L={L}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs
    if isinstance(m, nn.ConvTranspose1d):  # the (B, C, L) module boundary, both grad modes
        with torch.no_grad():
            assert rel_l2(m(_dev(x)), ry) < TOL
        assert rel_l2(m(_dev(x)), ry) < TOL
