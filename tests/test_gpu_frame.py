"""The 2-D virtual-frame kernels against an fp64 reference of the same operation.

A U-Net block reads its input as a virtual frame: up to three NHWC sources, each at its own (possibly negative)
offset, concatenated along channels, then GroupNorm and GELU.  Pinned here, at unit size:

  nps_group_norm_stats  gn_stats_kernel / gn_accum_src (whole rows, channel-quad sub-range, scalar)
  nps_stats_sum         stats_sum_kernel
  nps_frame_pack        frame_pack_kernel (flat, 4-aligned multi-source, generic fetch4 + out_C padding)
  nps_frame_pack_bwd*   frame_bwd_reduce[4]_kernel, frame_bwd_apply[4]_kernel, frame_bwd_s12 and the host dispatch
                        (quad / scalar by channel counts and pointer alignment, 64 / 128 / 256 pixels per block)

Reference: the dense frame built in fp64 on the CPU by index arithmetic, act(F.group_norm(frame)) and fp64 torch
autograd of that expression.  Bars: moments rtol 1e-6 / atol 1e-3 (the 3-D moments' bar), forward rel-L2 < 1e-6
(fp32 quad partials, fp64 sums, fp32 (mean, rstd) emulate to 1-2e-7), gradients rel-L2 < 1e-5 (the project's
gradient bar).
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-6
GRAD_TOL = 1e-5
EPS = 1e-5

# id -> (frame (H, W), [(C, H, W, off_y, off_x), ...], GroupNorm groups, (mean, std) of the inputs)
FRAME = (13, 17)
CASES = {
    # quad kernels, G = 1; moments: whole rows (sources 0, 1) and quad sub-range (the cropped source 2);
    # uncovered frame pixels (source 1) and cropped-away source pixels (source 2)
    "A": (FRAME, [(20, 13, 17, 0, 0), (16, 10, 14, 1, 2), (4, 16, 20, -1, -2)], 1, (0.3, 1.5)),
    # the same with |mean| / std = 6
    "A_shift": (FRAME, [(20, 13, 17, 0, 0), (16, 10, 14, 1, 2), (4, 16, 20, -1, -2)], 1, (3.0, 0.5)),
    # the U-Net's final GroupNorm(8): 32 threads per group in frame_bwd_s12 (two groups per wave); flat frame_pack
    "B": (FRAME, [(32, 13, 17, 0, 0)], 8, (0.3, 1.5)),
    # 4 channels per group, 16 threads per group
    "C": (FRAME, [(64, 13, 17, 0, 0)], 16, (0.3, 1.5)),
    # 85 threads per group: mixed waves and the g >= G tail lane
    "D": (FRAME, [(24, 13, 17, 0, 0), (12, 13, 17, 2, -1)], 3, (0.3, 1.5)),
    # ... and with the middle group [12, 24) across the source boundary at channel 20 (quad kernels)
    "D_straddle": (FRAME, [(20, 13, 17, 0, 0), (16, 13, 17, 2, -1)], 3, (0.3, 1.5)),
    # 5 channels per group: scalar backward kernels with 4-aligned sources
    "E": (FRAME, [(40, 13, 17, 0, 0)], 8, (0.3, 1.5)),
    # scalar kernels, groups across sources off the quad; generic frame_pack path
    "F_g3": (FRAME, [(6, 13, 17, 0, 0), (4, 15, 19, -1, -1), (2, 11, 15, 1, 1)], 3, (0.3, 1.5)),
    "F_g2": (FRAME, [(6, 13, 17, 0, 0), (4, 15, 19, -1, -1), (2, 11, 15, 1, 1)], 2, (0.3, 1.5)),
    # 11 channels: out_C = 12, one pad channel
    "F_pad": (FRAME, [(6, 13, 17, 0, 0), (4, 15, 19, -1, -1), (1, 11, 15, 1, 1)], 1, (0.3, 1.5)),
    # Q = 1 / 2 channel quads: a thread's pixel stride (256 / 128) above the block's pixels (64) and the row width
    "G_c4": (FRAME, [(4, 13, 17, 0, 0)], 1, (0.3, 1.5)),
    "G_c8": (FRAME, [(8, 13, 17, 0, 0)], 1, (0.3, 1.5)),
    # the up-block's 388-channel frame: Q = 97 (per = 2, 62 idle threads)
    "H": ((9, 11), [(192, 9, 11, 0, 0), (192, 9, 11, 0, 0), (4, 12, 14, -1, -2)], 1, (0.3, 1.5)),
    # 501 blocks x B = 2 >= 1000: 256 pixels per block
    "I": ((362, 354), [(8, 362, 354, 0, 0)], 2, (0.3, 1.5)),
    # 350 blocks x 2 < 1000 <= 699 blocks x 2: 128 pixels per block
    "I_px128": ((300, 298), [(8, 300, 298, 0, 0)], 2, (0.3, 1.5)),
    # A's sources, each overlapping the frame on one side per axis
    "J": (FRAME, [(20, 13, 17, 0, 0), (16, 10, 14, -2, 3), (4, 16, 20, 3, -2)], 1, (0.3, 1.5)),
}
MODES = {"gn_gelu": (True, 1), "gn": (True, 0), "gelu": (False, 1), "plain": (False, 0)}
B = 2


# ------------------------------------------------------------------ reference
def dense_frame(srcs, offs, hw):
    """fp64 dense frame (B, sum C, H, W) of NCHW sources: frame pixel (y, x) of a source's channel block is source
    pixel (y - off_y, x - off_x) where that lies inside the source, else 0.  Differentiable."""
    H, W = hw
    fr = torch.zeros((srcs[0].shape[0], sum(s.shape[1] for s in srcs), H, W), dtype=torch.float64)
    lo = 0
    for s, (oy, ox) in zip(srcs, offs):
        C, Hs, Ws = s.shape[1:]
        y0, y1 = max(0, oy), min(H, oy + Hs)
        x0, x1 = max(0, ox), min(W, ox + Ws)
        if y0 < y1 and x0 < x1:
            fr[:, lo:lo + C, y0:y1, x0:x1] = s[:, :, y0 - oy:y1 - oy, x0 - ox:x1 - ox].double()
        lo += C
    return fr


def in_frame_mask(shape, off, hw):
    """(Hs, Ws) bool: source pixels whose frame position lies inside the frame."""
    _, Hs, Ws = shape
    ys = torch.arange(Hs) + off[0]
    xs = torch.arange(Ws) + off[1]
    return ((ys >= 0) & (ys < hw[0]))[:, None] & ((xs >= 0) & (xs < hw[1]))[None, :]


def covered_mask(case):
    """(Cin, H, W) bool: frame elements that a source covers."""
    hw, specs, _, _ = CASES[case]
    ones = [torch.ones((1, c, h, w)) for c, h, w, _, _ in specs]
    return dense_frame(ones, [(oy, ox) for *_, oy, ox in specs], hw)[0] > 0


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The case's tensors, made once on the CPU: NCHW fp32 sources, gamma, beta, two output gradients."""
    hw, specs, G, (mean, std) = CASES[case]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    c = Inputs()
    c.hw, c.G = hw, G
    c.offs = tuple((oy, ox) for *_, oy, ox in specs)
    c.srcs = [torch.randn((B, ch, h, w), generator=g) * std + mean for ch, h, w, _, _ in specs]
    c.Cin = sum(s.shape[1] for s in c.srcs)
    c.gamma = 1 + 0.2 * torch.randn(c.Cin, generator=g)
    c.beta = 0.1 * torch.randn(c.Cin, generator=g)
    c.g1 = torch.randn((B, c.Cin, *hw), generator=g)
    c.g2 = torch.randn((B, c.Cin, *hw), generator=g)
    return c


def reference(case, mode, use_out=True, use_plain=False):
    """fp64: out = act(GN(frame)), and the gradients of sum(g1 out) [+ sum(g2 frame)] by torch autograd."""
    c = inputs(case)
    has_gn, act = MODES[mode]
    xs = [s.double().requires_grad_(True) for s in c.srcs]
    gamma, beta = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    fr = dense_frame(xs, c.offs, c.hw)
    out = F.group_norm(fr, c.G, gamma, beta, EPS) if has_gn else fr
    if act:
        out = F.gelu(out)
    loss = 0
    if use_out:
        loss = loss + (c.g1.double() * out).sum()
    if use_plain:
        loss = loss + (c.g2.double() * fr).sum()
    loss.backward()
    r = Inputs()
    r.frame, r.out = fr.detach(), out.detach()
    r.dsrc = [x.grad for x in xs]
    r.dgamma, r.dbeta = gamma.grad, beta.grad
    return r


@functools.lru_cache(maxsize=None)
def reference_out(case, mode):
    return reference(case, mode)


@functools.lru_cache(maxsize=None)
def affine_noise(case, mode):
    """Per channel, how far two fp32 evaluations of dgamma_c = sum gz xhat and dbeta_c = sum gz (gz = g1 act'(z), over
    every pixel and sample) may differ: 16 x 2^-24 x the sum of the terms' magnitudes.  Each term carries a few fp32
    roundings (<= 8 x 2^-24 relative) and each addition rounds at 2^-24 of a partial sum that stays below sum |term|;
    the kernels chain at most 64 terms per register before combining partials, and the roundings do not align, so
    this sits an order of magnitude above what two summation orders give (measured: 1.7e-6 on a dbeta element of
    3.8e-3 whose terms sum to ~100 in magnitude) and four below the size of one dropped term."""
    c = inputs(case)
    _, act = MODES[mode]
    fr = reference_out(case, mode).frame
    xh = F.group_norm(fr, c.G, None, None, EPS)
    z = xh * c.gamma.double()[None, :, None, None] + c.beta.double()[None, :, None, None]
    gz = c.g1.double()
    if act:
        gz = gz * (0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
    k = 16 * 2.0 ** -24
    return k * (gz * xh).abs().sum((0, 2, 3)), k * gz.abs().sum((0, 2, 3))


def affine_same(case, mode, dg_a, db_a, dg_b, db_b):
    """dgamma / dbeta of two runs of the frame backward (other kernels, or another order of the float atomics)."""
    ng, nb = affine_noise(case, mode)
    for a, b, noise in ((dg_a, dg_b, ng), (db_a, db_b, nb)):
        a, b = a.cpu().double(), b.cpu().double()
        assert bool(((a - b).abs() <= 1e-5 * b.abs() + noise).all()), ((a - b).abs().max().item(), noise.min().item())


# ------------------------------------------------------------------ device side
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).cpu()


def dev_srcs(case):
    from nps_hip import ops
    c = inputs(case)
    return [ops.Src(nhwc(s), oy, ox) for s, (oy, ox) in zip(c.srcs, c.offs)]


def stats_ctypes(srcs, hw, Cin, G, stats=None, zero_first=1):
    """nps_group_norm_stats through ctypes (ops.group_norm_stats short-cuts G = 1 with sources inside the frame)."""
    from nps_hip import ops, lib, ptr, stream_ptr, check
    if stats is None:
        stats = torch.full((B, G, 2), float("nan"), dtype=torch.float64, device=DEV)
    check(lib.nps_group_norm_stats(ops._c_src(srcs), len(srcs), B, hw[0], hw[1], Cin, G, ptr(stats), zero_first,
                                   stream_ptr()), "group_norm_stats")
    return stats


def ref_moments(fr, G):
    x = fr.reshape(fr.shape[0], G, -1)
    return torch.stack([x.sum(-1), (x * x).sum(-1)], dim=-1)


def frame_args(srcs, hw, Cin, gn=None, act=0):
    """nps_conv2d_t of a frame; gn = (stats, gamma, beta, groups) device tensors or None."""
    from nps_hip import ops, ptr, Conv2dArgs
    a = Conv2dArgs()
    a.nsrc, a.src = len(srcs), ops._c_src(srcs)
    a.B, a.Hin, a.Win, a.Cin = B, hw[0], hw[1], Cin
    if gn is not None:
        a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_groups, a.gn_eps = ptr(gn[0]), ptr(gn[1]), ptr(gn[2]), gn[3], EPS
    a.pre_act = act
    return a


GUARD = 64  # floats (256 B: a slice behind the guard keeps the buffer's 16-B alignment)


def guarded(n, skew=0, dtype=torch.float32):
    """(buffer, slice): n elements `skew` elements off 16-B alignment inside a NaN-filled buffer, guards both sides."""
    big = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=dtype, device=DEV)
    return big, big[GUARD + skew:GUARD + skew + n]


def guards_intact(big, n, skew=0):
    lo, hi = big[:GUARD + skew], big[GUARD + skew + n:]
    return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())


def run_bwd(case, mode, entry="bwd", gy_skew=0, plain=False):
    """nps_frame_pack_bwd / _bwd2 through ctypes into NaN-guarded outputs.  Returns (dsrc list NHWC, dgamma, dbeta)
    after checking that every output element was written and no guard float was."""
    from nps_hip import lib, ptr, stream_ptr, check
    c = inputs(case)
    has_gn, act = MODES[mode]
    srcs = dev_srcs(case)
    gamma, beta = c.gamma.to(DEV), c.beta.to(DEV)
    gn = (stats_ctypes(srcs, c.hw, c.Cin, c.G), gamma, beta, c.G) if has_gn else None
    a = frame_args(srcs, c.hw, c.Cin, gn, act)
    n = B * c.hw[0] * c.hw[1] * c.Cin
    gy_big = torch.zeros(n + 8, device=DEV)
    gy = gy_big[gy_skew:gy_skew + n]
    gy.copy_(nhwc(c.g1).reshape(-1))
    assert gy.data_ptr() % 16 == 4 * gy_skew
    gp = nhwc(c.g2) if plain else None
    outs = [guarded(s.t.numel()) for s in srcs]
    dg_big, dg = guarded(c.Cin)
    db_big, db = guarded(c.Cin)
    arr = (ctypes.c_void_p * 3)(*[o[1].data_ptr() for o in outs] + [None] * (3 - len(outs)))
    if entry == "bwd":  # zeroes `work` itself
        work = torch.full((B, 2, c.Cin), 1e30, dtype=torch.float64, device=DEV)
        check(lib.nps_frame_pack_bwd(ctypes.byref(a), gy.data_ptr(), arr, ptr(dg), ptr(db), ptr(work), stream_ptr()),
              "frame_pack_bwd")
    else:               # expects `work` zeroed
        work = torch.zeros((B, 2, c.Cin), dtype=torch.float64, device=DEV)
        check(lib.nps_frame_pack_bwd2(ctypes.byref(a), gy.data_ptr(), ptr(gp), arr, None, ptr(dg), ptr(db), ptr(work),
                                      stream_ptr()), "frame_pack_bwd2")
    torch.cuda.synchronize()
    for (big, view), s in zip(outs, srcs):
        assert not torch.isnan(view).any(), "source gradient elements left unwritten"
        assert guards_intact(big, s.t.numel()), "write outside the source gradient"
    if has_gn:
        for big, view in ((dg_big, dg), (db_big, db)):
            assert not torch.isnan(view).any() and guards_intact(big, c.Cin)
    else:  # no GroupNorm: the affine gradients do not exist and must stay untouched
        assert torch.isnan(dg_big).all() and torch.isnan(db_big).all()
    return [v.view(s.t.shape) for (_, v), s in zip(outs, srcs)], dg, db


def check_affine_grads(ref, dsrc_got, dgamma, dbeta):
    """dgamma / dbeta at rel-L2 < 1e-5 each; one that cancels (a sum over every pixel) may instead pass the rule of
    test_gpu_backward._grads_ok over the whole gradient of the frame."""
    errs = (rel_l2(dgamma, ref.dgamma), rel_l2(dbeta, ref.dbeta))
    print(f"dgamma / dbeta: rel-L2 {errs[0]:.3e} / {errs[1]:.3e}")
    if max(errs) < GRAD_TOL:
        return
    from test_gpu_backward import _grads_ok
    named_ref = {f"src{i}": g for i, g in enumerate(ref.dsrc) if dsrc_got[i] is not None}
    named_got = {f"src{i}": nchw(g) for i, g in enumerate(dsrc_got) if g is not None}
    named_ref.update(gamma=ref.dgamma, beta=ref.dbeta)
    named_got.update(gamma=dgamma, beta=dbeta)
    _grads_ok(named_ref, named_got)


def check_source_grads(case, ref, got):
    c = inputs(case)
    for i, (g, want) in enumerate(zip(got, ref.dsrc)):
        if g is None:
            continue
        g = nchw(g)
        e = rel_l2(g, want)
        print(f"dsrc[{i}] {case}: rel-L2 {e:.3e}")
        assert e < GRAD_TOL, (case, i, e)
        outside = ~in_frame_mask(c.srcs[i].shape[1:], c.offs[i], c.hw)
        assert bool((g[:, :, outside] == 0).all()), f"source {i}: gradient outside the frame is not exactly 0"


# ------------------------------------------------------------------ forward: moments
@pytest.mark.parametrize("case", list(CASES))
def test_group_norm_stats_vs_fp64(case):
    """Per-group (sum, sum of squares) of the dense frame; then a call with zero_first = 0 onto known values adds."""
    c = inputs(case)
    srcs = dev_srcs(case)
    want = ref_moments(reference_out(case, "plain").frame, c.G)
    got = stats_ctypes(srcs, c.hw, c.Cin, c.G)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=1e-3)
    seed = torch.arange(B * c.G * 2, dtype=torch.float64).view(B, c.G, 2) * 3.0 - 7.0
    acc = stats_ctypes(srcs, c.hw, c.Cin, c.G, stats=seed.to(DEV), zero_first=0)
    torch.testing.assert_close(acc.cpu(), seed + want, rtol=1e-6, atol=1e-3)


def test_group_norm_stats_carried_moments_g1():
    """ops.group_norm_stats with G = 1 and every source inside the frame: the sources' carried moments summed by
    nps_stats_sum give the numbers of the frame pass."""
    from nps_hip import ops
    g = torch.Generator().manual_seed(7)
    hw = FRAME
    specs = [(20, 13, 17, 0, 0), (16, 10, 14, 1, 2), (4, 9, 9, 4, 8)]
    xs = [torch.randn((B, ch, h, w), generator=g) * 1.5 + 0.3 for ch, h, w, _, _ in specs]
    offs = [(oy, ox) for *_, oy, ox in specs]
    srcs = [ops.Src(nhwc(x), *o) for x, o in zip(xs, offs)]
    want = ref_moments(dense_frame(xs, offs, hw), 1)
    assert all(ops.stats_of(s.t) is None for s in srcs)
    got = ops.group_norm_stats(srcs, hw, 1)
    assert all(ops.stats_of(s.t) is not None for s in srcs)  # (the carried-moments path ran)
    assert got.shape == (B, 1, 2)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=1e-3)
    direct = stats_ctypes(srcs, hw, 40, 1)
    torch.testing.assert_close(got.cpu(), direct.cpu(), rtol=1e-6, atol=1e-3)
    again = ops.group_norm_stats(srcs, hw, 1)  # now from the carried moments alone
    assert torch.equal(again, got)


@pytest.mark.parametrize("n_out", [16, 1])
def test_stats_sum_direct(n_out):
    """nps_stats_sum: slot 0 of the output = the sum over all parts' sub-slots; the other slots stay."""
    from nps_hip import lib, ptr, stream_ptr, check
    g = torch.Generator().manual_seed(3)
    nb = 3
    parts = [torch.rand((nb, n, 2), generator=g, dtype=torch.float64) + 0.5 for n in (16, 1, 3)]  # (no cancellation)
    dev = [p.to(DEV) for p in parts]

    def exact(ps):
        return torch.tensor([[math.fsum(v for p in ps for v in p[b, :, k].tolist()) for k in range(2)]
                             for b in range(nb)], dtype=torch.float64)

    for k in (3, 1):  # all three parts; p1 = p2 = NULL
        out = torch.full((nb, n_out, 2), -12345.0, dtype=torch.float64, device=DEV)
        p = dev[:k] + [None] * (3 - k)
        check(lib.nps_stats_sum(ptr(p[0]), 16, ptr(p[1]), 1 if k > 1 else 0, ptr(p[2]), 3 if k > 1 else 0, nb,
                                ptr(out), n_out, stream_ptr()), "stats_sum")
        torch.testing.assert_close(out[:, 0].cpu(), exact(parts[:k]), rtol=1e-14, atol=0)
        assert bool((out[:, 1:] == -12345.0).all())


# ------------------------------------------------------------------ forward: frame_pack
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_frame_pack_vs_fp64(case, mode):
    from nps_hip import ops
    c = inputs(case)
    has_gn, act = MODES[mode]
    ref = reference_out(case, mode)
    srcs = dev_srcs(case)
    gn = None
    if has_gn:
        gn = ops.GN(ops.group_norm_stats(srcs, c.hw, c.G), c.gamma.to(DEV), c.beta.to(DEV), c.G, EPS)
    pad4 = case.startswith("F_")
    out = ops.frame_pack(srcs, c.hw, gn, act, pad4=pad4)
    oC = (c.Cin + 3) // 4 * 4 if pad4 else c.Cin
    assert out.shape == (B, *c.hw, oC)
    assert ops.tag_value(out) == float(out.abs().max())
    if oC > c.Cin:
        assert case == "F_pad" and bool((out[..., c.Cin:] == 0).all()), "pad channels must be exactly 0.0"
    got = nchw(out[..., :c.Cin])
    e = rel_l2(got, ref.out)
    print(f"frame_pack {case} {mode}: rel-L2 {e:.3e}")
    assert e < FWD_TOL, (case, mode, e)
    # uncovered frame elements: act(gamma_c (0 - mu) rstd + beta_c), one value per (sample, channel).  The reference
    # holds exactly that; ~8 fp32 roundings of terms bounded by 1 + |z| (erff within a few ulp) sit below
    # 16 x 2^-24 x (1 + |z|).
    unc = ~covered_mask(case)
    if bool(unc.any()):
        g, r = got[:, unc].double(), ref.out[:, unc]
        if not has_gn:
            assert bool((g == 0).all())
        else:
            assert bool(((g - r).abs() <= 16 * 2.0 ** -24 * (1 + r.abs())).all())
        for ch in range(c.Cin):  # (the same arithmetic on the same operands: bit-equal within a channel)
            if bool(unc[ch].any()):
                v = got[:, ch][:, unc[ch]]
                assert bool((v == v[:, :1]).all())


# ------------------------------------------------------------------ backward: autograd functions
def run_frame_fn(case, mode, pair=False, use_out=True, use_plain=False, no_grad=()):
    """FrameFn / FramePairFn forward + backward on the device; returns (dsrc list or None entries, dgamma, dbeta,
    outputs)."""
    from nps_hip import autograd as ad
    c = inputs(case)
    has_gn, act = MODES[mode]
    xs = [nhwc(s).requires_grad_(i not in no_grad) for i, s in enumerate(c.srcs)]
    gamma = c.gamma.to(DEV).requires_grad_(True) if has_gn else None
    beta = c.beta.to(DEV).requires_grad_(True) if has_gn else None
    meta = (c.offs, c.hw, c.G if has_gn else 0, EPS if has_gn else 0.0, act)
    if pair:
        out, plain = ad.FramePairFn.apply(meta, gamma, beta, *xs)
        loss = 0
        if use_out:
            loss = loss + (nhwc(c.g1) * out).sum()
        if use_plain:
            loss = loss + (nhwc(c.g2) * plain).sum()
        outs = (out, plain)
    else:
        out = ad.FrameFn.apply(meta, gamma, beta, *xs)
        loss = (nhwc(c.g1) * out).sum()
        outs = (out,)
    loss.backward()
    return ([x.grad for x in xs], gamma.grad if has_gn else None, beta.grad if has_gn else None, outs, xs)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_frame_fn_backward_vs_fp64(case, mode):
    """FrameFn: every source gradient, dgamma and dbeta against fp64 autograd of act(GN(dense frame))."""
    ref = reference_out(case, mode)
    dsrc, dg, db, (out,), _ = run_frame_fn(case, mode)
    assert rel_l2(nchw(out), ref.out) < FWD_TOL
    check_source_grads(case, ref, dsrc)
    if MODES[mode][0]:
        check_affine_grads(ref, dsrc, dg, db)


PAIR_CASES = ["A", "B", "D_straddle", "F_g3", "H"]


@pytest.mark.parametrize("mode", ["gn_gelu", "gelu"])
@pytest.mark.parametrize("case", PAIR_CASES)
def test_frame_pair_fn_both_outputs(case, mode):
    """FramePairFn, loss = sum(g1 out) + sum(g2 plain): the plain output's gradient is added inside the frame
    backward (gy_plain).  A single covering source is returned as the plain output itself (`ident`)."""
    c = inputs(case)
    ref = reference(case, mode, use_out=True, use_plain=True)
    dsrc, dg, db, (out, plain), xs = run_frame_fn(case, mode, pair=True, use_out=True, use_plain=True)
    assert rel_l2(nchw(out), ref.out) < FWD_TOL
    assert torch.equal(nchw(plain).double(), ref.frame), "the plain output is a pure gather: exact"
    ident = len(c.srcs) == 1
    assert (plain.data_ptr() == xs[0].data_ptr()) == ident
    check_source_grads(case, ref, dsrc)
    if MODES[mode][0]:
        check_affine_grads(ref, dsrc, dg, db)


@pytest.mark.parametrize("case", PAIR_CASES)
def test_frame_pair_fn_plain_output_only(case):
    """FramePairFn with only the plain output used: the source gradients are the gather of g2 (exact), the affine
    gradients exactly 0."""
    c = inputs(case)
    ref = reference(case, "gn_gelu", use_out=False, use_plain=True)
    dsrc, dg, db, _, _ = run_frame_fn(case, "gn_gelu", pair=True, use_out=False, use_plain=True)
    check_source_grads(case, ref, dsrc)
    for g, want in zip(dsrc, ref.dsrc):
        assert torch.equal(nchw(g).double(), want)
    assert dg is None or bool((dg == 0).all())
    assert db is None or bool((db == 0).all())
    assert ref.dgamma is None or bool((ref.dgamma == 0).all())
    assert len(c.srcs) == len(dsrc)


@pytest.mark.parametrize("case,skip", [("A", 0), ("A", 2), ("F_g3", 0), ("F_g3", 2)])
def test_frame_fn_source_without_gradient(case, skip):
    """A source with requires_grad = False (dsrc[i] == NULL), first and last: no gradient for it, the other
    gradients and dgamma / dbeta as with all sources differentiated."""
    ref = reference_out(case, "gn_gelu")
    full = run_frame_fn(case, "gn_gelu")
    dsrc, dg, db, _, _ = run_frame_fn(case, "gn_gelu", no_grad=(skip,))
    assert dsrc[skip] is None
    check_source_grads(case, ref, dsrc)
    check_affine_grads(ref, dsrc, dg, db)
    for i, g in enumerate(dsrc):  # (two runs differ by the order of the reduction's float atomics)
        if i != skip:
            torch.testing.assert_close(g, full[0][i], rtol=1e-5, atol=1e-6)
    affine_same(case, "gn_gelu", dg, db, full[1], full[2])


# ------------------------------------------------------------------ backward: C ABI
@pytest.mark.parametrize("mode", ["gn_gelu", "plain"])
@pytest.mark.parametrize("case", ["A", "C", "F_g3", "G_c4", "H"])
def test_frame_pack_bwd_abi_guards_alignment_and_work(case, mode):
    """nps_frame_pack_bwd / nps_frame_pack_bwd2 into slices of NaN-filled buffers: every element written, no guard
    float touched (run_bwd); a gy 4 bytes off 16-B alignment must take the scalar kernels and agree; the entry that
    zeroes `work` itself (handed garbage) and the one that expects it zeroed agree.  Source gradients agree within
    rtol 1e-5 / atol 1e-6 (two runs that differ by the order of float atomics, as the tagged-vs-untagged test);
    dgamma / dbeta are fp32 sums over every pixel, which another kernel adds in another order: each run is held to
    fp64 at the gradient bar, and the runs to each other within affine_noise."""
    ref = reference_out(case, mode)
    d0, dg0, db0 = run_bwd(case, mode, "bwd")
    check_source_grads(case, ref, d0)
    d1, dg1, db1 = run_bwd(case, mode, "bwd", gy_skew=1)
    check_source_grads(case, ref, d1)
    d2, dg2, db2 = run_bwd(case, mode, "bwd2")
    has_gn = MODES[mode][0]
    for other, og, ob in ((d1, dg1, db1), (d2, dg2, db2)):
        for u, t in zip(d0, other):
            torch.testing.assert_close(u, t, rtol=1e-5, atol=1e-6)
        if has_gn:
            check_affine_grads(ref, other, og, ob)
            affine_same(case, mode, og, ob, dg0, db0)
    if has_gn:
        check_affine_grads(ref, d0, dg0, db0)


@pytest.mark.parametrize("case", ["A", "F_g3"])
def test_frame_pack_bwd2_gy_plain_abi(case):
    """nps_frame_pack_bwd2 with gy_plain through the C ABI against fp64 (guards as above)."""
    ref = reference(case, "gn_gelu", use_out=True, use_plain=True)
    d, dg, db = run_bwd(case, "gn_gelu", "bwd2", plain=True)
    check_source_grads(case, ref, d)
    check_affine_grads(ref, d, dg, db)


def test_frame_entry_points_refuse_bad_arguments():
    """Bad arguments return < 0 with a message in nps_last_error and launch nothing: the outputs keep their NaNs."""
    from nps_hip import lib, ptr, stream_ptr
    case = "E"  # 40 channels
    c = inputs(case)
    srcs = dev_srcs(case)
    gamma, beta = c.gamma.to(DEV), c.beta.to(DEV)
    stats = stats_ctypes(srcs, c.hw, c.Cin, c.G)
    n = B * c.hw[0] * c.hw[1]
    gy = nhwc(c.g1)

    def bad_args(kind):
        a = frame_args(srcs, c.hw, c.Cin, (stats, gamma, beta, c.G), 1)
        if kind == "cin":
            a.Cin = c.Cin + 1           # sum of C_i != Cin
        elif kind == "g17":
            a.gn_groups = 17
        elif kind == "gdiv":
            a.gn_groups = 3             # 40 % 3 != 0
        elif kind == "outc":
            a.out_C = c.Cin + 4
        return a

    def refused(rc, what):
        msg = lib.nps_last_error().decode()
        assert rc < 0 and what in msg, (rc, msg)

    for kind in ("cin", "g17", "gdiv", "outc"):
        out = torch.full((n * (c.Cin + 4),), float("nan"), device=DEV)
        refused(lib.nps_frame_pack(ctypes.byref(bad_args(kind)), ptr(out), stream_ptr()), "frame_pack")
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    for kind in ("cin", "g17", "gdiv"):
        a = bad_args(kind)
        d = torch.full_like(srcs[0].t, float("nan"))
        dg, db = torch.full((c.Cin + 4,), float("nan"), device=DEV), torch.full((c.Cin + 4,), float("nan"), device=DEV)
        work = torch.full((B, 2, c.Cin + 4), float("nan"), dtype=torch.float64, device=DEV)
        arr = (ctypes.c_void_p * 3)(d.data_ptr(), None, None)
        refused(lib.nps_frame_pack_bwd(ctypes.byref(a), ptr(gy), arr, ptr(dg), ptr(db), ptr(work), stream_ptr()),
                "frame_pack_bwd")
        refused(lib.nps_frame_pack_bwd2(ctypes.byref(a), ptr(gy), None, arr, None, ptr(dg), ptr(db), ptr(work),
                                        stream_ptr()), "frame_pack_bwd")
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (d, dg, db, work))
    from nps_hip import ops
    st = torch.full((B, c.G, 2), float("nan"), dtype=torch.float64, device=DEV)
    refused(lib.nps_group_norm_stats(ops._c_src(srcs), 1, B, c.hw[0], c.hw[1], c.Cin + 1, c.G, ptr(st), 1,
                                     stream_ptr()), "group_norm_stats")
    refused(lib.nps_group_norm_stats(ops._c_src(srcs), 1, B, c.hw[0], c.hw[1], c.Cin, 3, ptr(st), 1, stream_ptr()),
            "group_norm_stats")
    torch.cuda.synchronize()
    assert torch.isnan(st).all()
