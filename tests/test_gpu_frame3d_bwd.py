"""The 3-D frame kernels (csrc/frame3d_bwd.hip: nps_frame3d_fwd / nps_frame3d_bwd / nps_add_at_copy3d) and Conv3dFn at
the channel counts the 3-D U-Net walk brings, against torch CPU fp64 autograd.

Frame reference: gelu(group_norm(cat(crop_nd(src_i)))) under a random cotangent gy; where gy_plain is tested,
(cat(crop_nd(src_i)) * g2).sum() is added to the loss.  rel-L2 < 1e-5 for y, each dsrc, dgamma and dbeta: the
project's fp32 bar (tests/test_gpu_conv3d_bwd.py, tests/test_gpu_backward.py).  B = 2 (per-sample tables are indexed),
frame (5, 6, 7) = 210 voxels (no multiple of a block or unroll step), sizes and offsets distinct per axis."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
B = 2
FRAME = (5, 6, 7)
# src0 is exact; src1 is cropped on D and H; src2 is zero-padded on D and H and cropped on W
GEO = {1: [(FRAME, (0, 0, 0))],
       3: [(FRAME, (0, 0, 0)), ((7, 9, 8), (-1, -2, 0)), ((3, 4, 9), (1, 1, -1))]}


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.float32)


def _ncdhw(t):
    return t.detach().cpu().permute(0, 4, 1, 2, 3).double()


def _ranges(dhw, off, frame):
    """Per axis (frame range, source range) of crop_Nd's overlap."""
    out = []
    for n, o, f in zip(dhw, off, frame):
        f0, f1 = max(0, o), min(f, o + n)
        out.append((slice(f0, f1), slice(f0 - o, f1 - o)))
    return out


def _place(x, off, frame):
    """crop_Nd with explicit offsets on NCDHW: x placed at `off` inside a zero frame (differentiable)."""
    (fd, sd), (fh, sh), (fw, sw) = _ranges(x.shape[2:], off, frame)
    out = torch.zeros(x.shape[:2] + tuple(frame), dtype=x.dtype)
    out[:, :, fd, fh, fw] = x[:, :, sd, sh, sw]
    return out


def _outside(dhw, off, frame):
    """Bool (D, H, W): the source voxels that lie outside the frame."""
    m = torch.ones(dhw, dtype=torch.bool)
    (_, sd), (_, sh), (_, sw) = _ranges(dhw, off, frame)
    m[sd, sh, sw] = False
    return m


@functools.lru_cache(maxsize=None)
def _case(Cs, G, act, plain, seed=0):
    """fp32-representable operands and the fp64 reference (y, [dsrc], dgamma, dbeta), once per case."""
    g = torch.Generator().manual_seed(seed)
    geo = GEO[len(Cs)]
    Cin = sum(Cs)
    xs = [torch.randn(B, C, *dhw, generator=g) + 0.5 for C, (dhw, _) in zip(Cs, geo)]
    gamma = 1 + 0.3 * torch.randn(Cin, generator=g)
    beta = 0.2 * torch.randn(Cin, generator=g)
    gy = torch.randn(B, Cin, *FRAME, generator=g)
    g2 = torch.randn(B, Cin, *FRAME, generator=g) if plain else None
    xd = [x.double().requires_grad_(True) for x in xs]
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    cat = torch.cat([_place(x, off, FRAME) for x, (_, off) in zip(xd, geo)], dim=1)
    z = F.group_norm(cat, G, gd, bd, 1e-5) if G else cat
    y = F.gelu(z) if act else z
    loss = (y * gy.double()).sum()
    if plain:
        loss = loss + (cat * g2.double()).sum()
    loss.backward()
    return xs, gamma, beta, gy, g2, (y.detach(), [x.grad for x in xd], gd.grad, bd.grad)


def _run(Cs, G, act, plain, need=None):
    from nps_hip import ops
    xs, gamma, beta, gy, g2, ref = _case(Cs, G, act, plain)
    ss = [ops.Src3(_ndhwc(x), *off) for x, (_, off) in zip(xs, GEO[len(Cs)])]
    gn = None
    if G:
        gn = ops.GN(ops.gn_stats3d(ss, FRAME, G), gamma.to(DEV), beta.to(DEV), G, 1e-5)
    y = ops.frame3d(ss, FRAME, gn, act)
    assert y.shape == (B, *FRAME, sum(Cs))
    dsrc, dgamma, dbeta = ops.frame3d_bwd(ss, FRAME, gn, act, _ndhwc(gy), _ndhwc(g2) if plain else None, need)
    return y, dsrc, dgamma, dbeta, ref


def _check(Cs, G, act=1, plain=False):
    y, dsrc, dgamma, dbeta, (ry, rdx, rdg, rdb) = _run(Cs, G, act, plain)
    errs = dict(y=rel_l2(_ncdhw(y), ry))
    for i, (d, r) in enumerate(zip(dsrc, rdx)):
        errs[f"dsrc{i}"] = rel_l2(_ncdhw(d), r)
    if G:
        errs.update(dgamma=rel_l2(dgamma, rdg), dbeta=rel_l2(dbeta, rdb))
    else:
        assert dgamma is None and dbeta is None
    print(f"frame3d C={Cs} G={G} act={act} plain={plain}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    return dsrc


@pytest.mark.parametrize("C,G", [(16, 1), (16, 8), (32, 8)], ids=["c16g1_quad", "c16g8_generic", "c32g8_quad"])
def test_one_source(C, G):
    """One source covering the frame: GroupNorm(1) on quads, a group size of 2 (generic kernels), and the final
    norm's GroupNorm(8) with a group size of 4 (quads)."""
    _check((C,), G)


@pytest.mark.parametrize("Cs,G", [((16, 16, 2), 1), ((16, 16, 2), 2), ((16, 8, 4), 1)],
                         ids=["c34g1_generic", "c34g2_generic", "c28g1_quad"])
def test_three_sources_with_offsets(Cs, G):
    """Cropped and zero-padded sources: dsrc is exactly 0 at the source voxels outside the frame."""
    dsrc = _check(Cs, G)
    for i in (1, 2):
        dhw, off = GEO[3][i]
        out = _outside(dhw, off, FRAME).to(DEV)
        assert out.sum() > 0 and not out.all()
        assert (dsrc[i][:, out] == 0).all()
        assert (dsrc[i][:, ~out] != 0).any()


@pytest.mark.parametrize("act", [1, 0], ids=["gelu", "plain"])
@pytest.mark.parametrize("Cs", [(16, 16, 2), (16, 8, 4)], ids=["generic", "quad"])
def test_no_group_norm_with_gy_plain(Cs, act):
    _check(Cs, 0, act=act, plain=True)


@pytest.mark.parametrize("Cs", [(16, 16, 2), (16, 8, 4)], ids=["generic", "quad"])
def test_group_norm_with_gy_plain(Cs):
    _check(Cs, 1, plain=True)


def test_conditioning_without_gradient():
    """dsrc[2] = NULL (the conditioning requires no gradient): skipped, and the other outputs stay what they were
    (the fp64 atomic order of pass 1 may move a last bit: 1e-6, and the reference's bar)."""
    Cs = (16, 16, 2)
    _, full, fg, fb, _ = _run(Cs, 1, 1, False)
    _, dsrc, dgamma, dbeta, (_, rdx, rdg, rdb) = _run(Cs, 1, 1, False, need=[True, True, False])
    assert dsrc[2] is None
    for i in (0, 1):
        assert rel_l2(dsrc[i], full[i]) < 1e-6 and rel_l2(_ncdhw(dsrc[i]), rdx[i]) < TOL
    assert rel_l2(dgamma, fg) < 1e-6 and rel_l2(dbeta, fb) < 1e-6
    assert rel_l2(dgamma, rdg) < TOL and rel_l2(dbeta, rdb) < TOL


def test_frame3d_refuses_bf16():
    from nps_hip import ops
    x = torch.zeros(B, *FRAME, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32"):
        ops.frame3d([ops.Src3(x)], FRAME)


# ---------------------------------------------------------------- nps_add_at_copy3d / AddAt3dFn
@pytest.mark.parametrize("dhw,off", [((3, 4, 9), (1, 1, -1)), ((7, 9, 8), (-1, -2, 0))], ids=["pad", "crop"])
@pytest.mark.parametrize("C", [16, 18, 2])
def test_add_at3d(C, dhw, off):
    """out = base + crop_Nd(src) at the offset, and both gradients, against the torch construction."""
    from nps_hip import autograd as ad
    g = torch.Generator().manual_seed(C)
    base = torch.randn(B, C, *FRAME, generator=g)
    src = torch.randn(B, C, *dhw, generator=g)
    gy = torch.randn(B, C, *FRAME, generator=g)
    bd, sd = base.double().requires_grad_(True), src.double().requires_grad_(True)
    ref = bd + _place(sd, off, FRAME)
    (ref * gy.double()).sum().backward()
    bh, sh = _ndhwc(base).requires_grad_(True), _ndhwc(src).requires_grad_(True)
    out = ad.add_at3d(bh, sh, off)
    (out * _ndhwc(gy)).sum().backward()
    errs = dict(out=rel_l2(_ncdhw(out), ref.detach()), dbase=rel_l2(_ncdhw(bh.grad), bd.grad),
                dsrc=rel_l2(_ncdhw(sh.grad), sd.grad))
    print(f"add_at3d C={C} {dhw} at {off}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    outside = _outside(dhw, off, FRAME).to(DEV)
    assert (sh.grad[:, outside] == 0).all()


# ---------------------------------------------------------------- Conv3dFn off the 4-channel quads
@pytest.mark.parametrize("Cin,Cout,dhw,K,stride", [(18, 16, (5, 6, 7), 3, 1), (34, 16, (5, 6, 7), 1, 1),
                                                  (2, 2, (6, 7, 9), 3, 2)],
                         ids=["c18k3", "c34k1", "c2k3s2"])
def test_conv3d_fn_walk_channel_counts(Cin, Cout, dhw, K, stride):
    """The walk's frames have 18 / 34 channels with n_cond = 2, and conv_variables_broadcast is a 2 -> 2 stride-2
    conv (all valid): y, dx, dw, db against fp64."""
    from nps_hip import autograd as ad
    g = torch.Generator().manual_seed(Cin)
    x = torch.randn(B, Cin, *dhw, generator=g)
    w = torch.randn(Cout, Cin, K, K, K, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    ry = F.conv3d(xd, wd, bd, stride=stride)
    gy = torch.randn(ry.shape, generator=g)
    (ry * gy.double()).sum().backward()
    xh = _ndhwc(x).requires_grad_(True)
    wp, bp = nn.Parameter(w.to(DEV)), nn.Parameter(b.to(DEV))
    y = ad.Conv3dFn.apply((K, stride, 0, 0), xh, wp, bp)
    (y * _ndhwc(gy)).sum().backward()
    errs = dict(y=rel_l2(_ncdhw(y), ry.detach()), dx=rel_l2(_ncdhw(xh.grad), xd.grad), dw=rel_l2(wp.grad, wd.grad),
                db=rel_l2(bp.grad, bd.grad))
    print(f"Conv3dFn {Cin}->{Cout} K={K} s={stride}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
