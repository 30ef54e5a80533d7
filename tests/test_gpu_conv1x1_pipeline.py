"""The LDS-weight 1x1 split-fp16 conv (conv1x1_wl_kernel, conv2d_x3.hip) through ops.conv2d: every stage count
against the input ring depth and the two LDS weight buffers, every count of live 32-channel output blocks (the
branch-free 6-block path, the partial groups, the channel groups of Cout > 192 with their 1-block tail), the source
layouts, the epilogues, the fused GroupNorm + GELU prologue and the fused spectral W pass, against fp64 at the
suite's tolerance; and the outputs of a subset bit for bit against tests/golden/conv1x1_pipeline.pt, which
tools/gen_conv1x1_pipeline_golden.py wrote from the kernel before its main loop was software-pipelined (the
accumulation order of every output element is part of the kernel's contract)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
FRAMES = [(13, 17), (23, 37)]  # 221 and 851 pixels a sample: no multiple of the 128-pixel work-group tile
CINS = [20, 33, 64, 84, 96, 196, 388]  # 1, 2, 2, 3, 3, 7, 13 stages of 32 channels (196, 388: 4 live channels last)
COUTS = [192, 75, 160, 196, 388, 256]  # 6 blocks; 3 and 5 (ragged); 6 + 1, 6 + 6 + 1, 6 + 2


def _frame(srcs, H, W):
    """fp64 virtual frame (B, H, W, sum C) of sources (t, off_y, off_x): zero where a source does not cover."""
    parts = []
    for t, oy, ox in srcs:
        B, sH, sW, C = t.shape
        f = torch.zeros(B, H, W, C, dtype=torch.float64)
        y0, y1, x0, x1 = max(0, oy), min(H, oy + sH), max(0, ox), min(W, ox + sW)
        f[:, y0:y1, x0:x1] = t[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        parts.append(f)
    return torch.cat(parts, 3)


def _extend(f, pad, circ):
    if circ:
        f = torch.cat([f[:, -circ:], f, f[:, :circ]], 1)
        f = torch.cat([f[:, :, -circ:], f, f[:, :, :circ]], 2)
    if pad:
        f = F.pad(f, (0, 0, pad, pad, pad, pad))
    return f


def _case(seed=0, hw=(13, 17), chans=(96,), cout=192, offs=None, src_hw=None, pad=0, circ=0, bias=True, nadd=0,
          act=0, add_after_act=False, accumulate=False, out_c=None, stats=False, xscale=1.0):
    """Run one plain (no prologue) launch; returns dict(y, ref[, mom, mom_ref, spare])."""
    from nps_hip import ops
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(1000 + seed)
    offs = offs or [(0, 0)] * len(chans)
    src_hw = src_hw or [hw] * len(chans)
    srcs64 = [(torch.randn(B, sh[0], sh[1], c, generator=g, dtype=torch.float64) * xscale, o[0], o[1])
              for c, o, sh in zip(chans, offs, src_hw)]
    cin = sum(chans)
    w = torch.randn(cout, cin, generator=g, dtype=torch.float64) / cin ** 0.5
    b = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1 if bias else None
    Ho, Wo = H + 2 * (pad + circ), W + 2 * (pad + circ)
    # (an addend shares the output's layout: out_c channels a pixel when the output is strided)
    adds = [torch.randn(B, Ho, Wo, out_c or cout, generator=g, dtype=torch.float64) for _ in range(nadd)]
    prev = torch.randn(B, Ho, Wo, out_c or cout, generator=g, dtype=torch.float64) if (accumulate or out_c) else None
    # fp32 operands are what the kernel sees: the reference starts from their values
    srcs32 = [(t.float(), oy, ox) for t, oy, ox in srcs64]
    w32, b32 = w.float(), (b.float() if bias else None)
    adds32 = [a.float() for a in adds]
    v = _extend(_frame([(t.double(), oy, ox) for t, oy, ox in srcs32], H, W), pad, circ) @ w32.double().T
    if bias:
        v = v + b32.double()
    asum = sum(a.double()[..., :cout] for a in adds32) if adds else 0.0
    if not add_after_act:
        v = v + asum
    if act:
        v = F.gelu(v)
    if add_after_act:
        v = v + asum
    if accumulate:
        v = v + prev.float().double()[..., :cout]
    out = prev.float().to(DEV) if prev is not None else None
    ost = ops.new_stats(B, srcs32[0][0].to(DEV)) if stats else None
    wp = ops.pack_conv_weight(w32.view(cout, cin, 1, 1).to(DEV))
    y = ops.conv2d([ops.Src(t.to(DEV), oy, ox) for t, oy, ox in srcs32], hw, wp, b32.to(DEV) if bias else None, cout,
                   1, 1, pad=(pad, pad), circ=circ, addends=tuple(a.to(DEV) for a in adds32), act=act,
                   add_after_act=add_after_act, accumulate=accumulate, out=out, out_stats=ost)
    r = dict(y=y.cpu(), ref=v)
    if out_c:
        r["spare"], r["spare_ref"] = r["y"][..., cout:], prev.float()[..., cout:]
        r["y"] = r["y"][..., :cout].contiguous()
    if stats:
        assert not getattr(ost, "_nps_incomplete", False)
        r["mom"] = ost.sum(1).cpu()
        r["mom_ref"] = torch.stack([v.sum((1, 2, 3)), (v * v).sum((1, 2, 3))], 1)
    return r


def _pro_case(seed, cin, cout, groups, xscale, pad=0, hw=(13, 17)):
    """The GroupNorm + GELU prologue kernel (PRO): conv1x1(GELU(GroupNorm(x))) in one launch."""
    from nps_hip import ops
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(2000 + seed)
    x = (torch.randn(B, cin, H, W, generator=g) * xscale + 0.2 * xscale)
    gamma = torch.rand(cin, generator=g) + 0.5
    beta = torch.rand(cin, generator=g) - 0.5
    w = torch.randn(cout, cin, 1, 1, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(F.gelu(F.group_norm(x.double(), groups, gamma.double(), beta.double(), 1e-5)), w.double(),
                   b.double(), padding=pad)
    packs = []
    real_pack = ops.frame_pack
    try:
        ops.frame_pack = lambda *a, **k: packs.append(1) or real_pack(*a, **k)
        xd = ops.nchw_to_nhwc(x.to(DEV))
        st = ops.group_norm_stats([ops.Src(xd)], (H, W), groups)
        gn = ops.GN(st, gamma.to(DEV), beta.to(DEV), groups, 1e-5)
        y = ops.conv2d([ops.Src(xd)], (H, W), ops.pack_conv_weight(w.to(DEV)), b.to(DEV), cout, 1, 1, pad=(pad, pad),
                       gn=gn, pre_act=1)
    finally:
        ops.frame_pack = real_pack
    assert not packs, "the 1x1's GroupNorm prologue went through frame_pack"
    return dict(y=y.cpu(), ref=ref.permute(0, 2, 3, 1).contiguous())


BIG, SMALL = (23, 37), (13, 17)
# name -> (builder, kwargs).  Sources "larger than the frame with negative offsets" are crops (the U-Net's skips).
CASES = {
    "src2_crop": (_case, dict(seed=1, hw=BIG, chans=(192, 4), offs=[(-1, -2), (0, 0)], src_hw=[(26, 40), BIG])),
    "src3_crop": (_case, dict(seed=2, hw=SMALL, chans=(192, 192, 4), offs=[(-2, -1), (0, 0), (-1, -3)],
                              src_hw=[(16, 19), SMALL, (15, 21)])),
    "src_small": (_case, dict(seed=3, hw=BIG, chans=(64, 32), offs=[(0, 0), (3, 5)], src_hw=[BIG, (11, 19)], cout=160)),
    "pad1": (_case, dict(seed=4, hw=SMALL, chans=(84,), pad=1, cout=75, bias=True)),
    "circ1": (_case, dict(seed=5, hw=BIG, chans=(96,), circ=1)),
    "circ1_pad1_groups": (_case, dict(seed=6, hw=SMALL, chans=(192, 4), circ=1, pad=1, cout=388)),
    "plain_nobias": (_case, dict(seed=7, hw=BIG, chans=(196,), bias=False)),
    "add_gelu": (_case, dict(seed=8, hw=BIG, chans=(96,), nadd=1, act=1)),
    "gelu_add": (_case, dict(seed=9, hw=SMALL, chans=(196,), nadd=1, act=1, add_after_act=True, cout=160)),
    "add_gelu_groups": (_case, dict(seed=10, hw=SMALL, chans=(64,), nadd=1, act=1, cout=196)),
    "stats": (_case, dict(seed=11, hw=BIG, chans=(196,), stats=True)),
    "stats_ragged": (_case, dict(seed=12, hw=SMALL, chans=(33,), stats=True, cout=76)),
    "two_adds_accumulate": (_case, dict(seed=13, hw=BIG, chans=(84,), nadd=2, accumulate=True)),
    "two_adds_gelu_after": (_case, dict(seed=14, hw=SMALL, chans=(196,), nadd=2, act=1, add_after_act=True, cout=256)),
    "accumulate_groups": (_case, dict(seed=15, hw=SMALL, chans=(96,), accumulate=True, cout=388)),
    "out_stride": (_case, dict(seed=16, hw=BIG, chans=(64,), out_c=200, nadd=1)),
    "out_stride_groups": (_case, dict(seed=17, hw=SMALL, chans=(20,), out_c=392, cout=388)),
    "scale_small": (_case, dict(seed=18, hw=SMALL, chans=(96,), xscale=1e-3)),
    "scale_large": (_case, dict(seed=19, hw=SMALL, chans=(196,), xscale=3e3, cout=75)),
    # GroupNorm divides Cin into the groups: 36 takes 1 and 3, 196 takes 1, the 8-group form runs at 64 and 192
    "pro_36_g3_small": (_pro_case, dict(seed=1, cin=36, cout=192, groups=3, xscale=1e-3)),
    "pro_36_g1_large": (_pro_case, dict(seed=2, cin=36, cout=75, groups=1, xscale=3e3, hw=BIG)),
    "pro_196_g1_small": (_pro_case, dict(seed=3, cin=196, cout=192, groups=1, xscale=1e-3, hw=BIG)),
    "pro_196_g1_large_pad": (_pro_case, dict(seed=4, cin=196, cout=160, groups=1, xscale=3e3, pad=1)),
    "pro_64_g8_small": (_pro_case, dict(seed=5, cin=64, cout=192, groups=8, xscale=1e-3)),
    "pro_192_g8_large": (_pro_case, dict(seed=6, cin=192, cout=192, groups=8, xscale=3e3, hw=BIG)),
}
for _i, _cin in enumerate(CINS):      # every stage count on the hot path, every block count at 3 stages and at 7
    CASES[f"cin{_cin}_cout192"] = (_case, dict(seed=30 + _i, hw=FRAMES[_i % 2], chans=(_cin,)))
for _i, _cout in enumerate(COUTS[1:]):
    CASES[f"cin96_cout{_cout}"] = (_case, dict(seed=40 + _i, hw=FRAMES[_i % 2], chans=(96,), cout=_cout))
    CASES[f"cin196_cout{_cout}"] = (_case, dict(seed=50 + _i, hw=FRAMES[(_i + 1) % 2], chans=(196,), cout=_cout))
for _i, (_cin, _cout) in enumerate([(20, 388), (33, 196), (64, 256), (84, 160), (388, 75), (388, 388), (388, 256),
                                    (20, 75), (33, 160), (64, 196), (84, 388)]):
    CASES[f"cin{_cin}_cout{_cout}"] = (_case, dict(seed=60 + _i, hw=FRAMES[_i % 2], chans=(_cin,), cout=_cout))

# the cases whose outputs the fixture pins bit for bit
BIT_CASES = ["cin20_cout192", "cin33_cout192", "cin96_cout192", "cin196_cout192", "cin388_cout192", "cin96_cout75",
             "cin196_cout160", "cin388_cout388", "cin196_cout196", "cin64_cout256", "src3_crop", "src_small", "circ1",
             "pad1", "add_gelu", "gelu_add", "two_adds_accumulate", "out_stride", "stats", "pro_36_g3_small",
             "pro_196_g1_large_pad", "pro_192_g8_large", "spec_36_44", "spec_196_192"]
BIT_FULL = ["cin96_cout75", "pad1", "spec_36_44"]  # stored whole; the others as exact digests (digest())


@functools.lru_cache(maxsize=None)
def run(name):
    """One launch per case and session: the fp64 and the bit-for-bit test read the same result."""
    if name.startswith("spec_"):
        return _spec_case(*[int(v) for v in name.split("_")[1:]])
    fn, kw = CASES[name]
    return fn(**kw)


def digest(y):
    """Exact, order-free digest of an fp32 tensor's bits: int64 sums of the int32 bit patterns along every axis
    but the last, and along the last.  Any changed bit of any element changes an entry of both."""
    bits = y.contiguous().view(torch.int32).to(torch.int64)
    flat = bits.reshape(-1, bits.shape[-1])
    return torch.cat([flat.sum(0), flat.sum(1)])


def _spec_case(cin, cout):
    """The FNO layer fusion: GELU(conv1x1(x) + b + W-pass synthesis of Z) in the 1x1's epilogue (nps_conv2d_t.spec_z)
    at the smallest eligible frame (one 128-pixel row per work-group), against the unfused launches and fp64."""
    from nps_hip import ops
    B, H, W, m2 = 2, 2, 128, 3
    assert ops.spectral_fusable(W, m2, cout)
    g = torch.Generator().manual_seed(3000 + cin)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    Z = torch.complex(torch.randn(B, H, m2, cout, generator=g), torch.randn(B, H, m2, cout, generator=g)) * 20.0
    scale = 1.0 / (H * W)
    Zp = torch.zeros(B, H, W // 2 + 1, cout, dtype=torch.complex128)
    Zp[:, :, :m2] = Z.to(torch.complex128)
    ref = F.gelu(x.double() @ w.double().T + b.double() + torch.fft.irfft(Zp, n=W, dim=2, norm="forward") * scale)
    wp = ops.pack_conv_weight(w.view(cout, cin, 1, 1).to(DEV))
    xd, bd, Zd = x.to(DEV), b.to(DEV), Z.to(DEV).contiguous()
    y = ops.conv2d([ops.Src(xd)], (H, W), wp, bd, cout, 1, 1, spec=(Zd, m2, scale), act=1)
    u = ops.conv2d([ops.Src(xd)], (H, W), wp, bd, cout, 1, 1)
    ops.check(ops.lib.nps_spectral_idft_w(ops.ptr(Zd), ops.ptr(u), B, H, W, m2, cout, 1, ops.ptr(None), 1,
                                          ops.out_tag(u, True), ops.stream_ptr()), "spectral_idft_w")
    # (idft_w applies 1 / (H W) itself: the scale irfft2's norm carries)
    return dict(y=y.cpu(), ref=ref, unfused=u.cpu())


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv1x1_wl_vs_fp64(name):
    r = run(name)
    assert r["y"].shape == r["ref"].shape
    err = rel_l2(r["y"], r["ref"])
    print(f"{name}: rel-L2 vs fp64 {err:.3e}")
    assert err < TOL
    if "mom" in r:  # out_stats: the moments of the stored values against fp64 sums
        merr = rel_l2(r["mom"], r["mom_ref"])
        print(f"{name}: moments rel-L2 {merr:.3e}")
        assert merr < TOL
    if "spare" in r:  # channels past Cout of a strided output stay untouched
        assert torch.equal(r["spare"], r["spare_ref"])


@pytest.mark.parametrize("cin,cout", [(36, 44), (196, 192)])
def test_conv1x1_wl_fused_spectral_synthesis(cin, cout):
    r = run(f"spec_{cin}_{cout}")
    e_ref, e_unf = rel_l2(r["y"], r["ref"]), rel_l2(r["y"], r["unfused"])
    print(f"spec {cin}->{cout}: vs fp64 {e_ref:.3e}, vs unfused {e_unf:.3e}")
    assert e_unf < 1e-6  # (the bound tests/test_gpu_parity.py::test_fno_layer_fused_synthesis holds the pair to)
    assert e_ref < TOL


@pytest.mark.parametrize("name", BIT_CASES)
def test_conv1x1_wl_bit_identical_to_fixture(name):
    gold = load_golden("conv1x1_pipeline")
    y = run(name)["y"]
    assert torch.equal(digest(y), gold["digest"][name])
    if name in BIT_FULL:
        assert torch.equal(y, gold["full"][name])
