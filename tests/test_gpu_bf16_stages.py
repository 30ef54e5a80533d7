"""Per-stage checks of the bf16-storage (C5) entry points: nps_f32_to_bf16 / nps_bf16_to_f32 bit for bit against
torch's CPU conversions, and nps_spectral_dft_w_bf16 / nps_spectral_idft_w_bf16 against fp64 on the same
bf16-rounded operands, so that only the kernel's own arithmetic and its one output rounding separate the two.
(nps_spectral_mix_bf16: test_gpu_spectral_mix.py.)  The composite tests of test_gpu_c5.py allow the bf16 rounding
of whole tensors (rel-L2 5e-3 / 1e-2), which hides truncation instead of round-to-nearest-even, a dropped Nyquist
rule or a mishandled source tail.
"""
import pytest
import torch

from conftest import rel_l2
from spectral2d_ref import c2r_partial as _c2r_partial

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _f32_bits(*words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


def _both_signs(words):
    return list(words) + [w | 0x80000000 for w in words]


# ------------------------------------------------------------------ conversions
def test_f32_to_bf16_bit_exact():
    """Round-to-nearest-even, bit for bit like torch's CPU conversion: a grid-stride tail, signed zeros, exact ties to
    even and to odd with their one-ulp neighbours, overflow to inf, infinities, the smallest normals; NaN stays NaN.
    fp32-subnormal inputs may be flushed: the RNE result or a zero of the input's sign is accepted.  Measured on an
    MI355X: all 18 subnormal inputs come out as the RNE result, none is flushed."""
    from nps_hip import ops
    g = torch.Generator().manual_seed(0)
    ties = [0x3F808000, 0x3F818000]                                  # 1 + 2^-8 (to even: down), 1 + 3 * 2^-8 (up)
    normal = _both_signs([0x00000000] + ties + [t - 1 for t in ties] + [t + 1 for t in ties] +
                         [0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000,      # max finite (-> inf), its tie, inf
                          0x00800000, 0x00808000, 0x00818000, 0x00FFFFFF])      # the smallest normals
    subnormal = _both_signs([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x00408000,
                             0x007F8000, 0x007FFFFF])                           # the last two round up to 2^-126
    nans = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F808000]
    x = torch.cat([torch.randn(4099, generator=g), _f32_bits(*normal), _f32_bits(*subnormal), _f32_bits(*nans)])
    n0, n1 = 4099 + len(normal), 4099 + len(normal) + len(subnormal)
    want = x.to(torch.bfloat16)
    got = ops.to_bf16(x.to(DEV)).cpu()
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    wb, gb = want.view(torch.int16), got.view(torch.int16)
    assert torch.equal(gb[:n0], wb[:n0]), (gb[:n0] != wb[:n0]).nonzero().flatten().tolist()
    assert want[n1:].isnan().all() and got[n1:].isnan().all()
    zero = (x[n0:n1].view(torch.int32) >> 31 << 15).to(torch.int16)  # 0x0000 / 0x8000 by the input's sign
    rne, flushed = gb[n0:n1] == wb[n0:n1], gb[n0:n1] == zero
    print(f"f32_to_bf16 of fp32 subnormals: {int(rne.sum())} of {n1 - n0} as RNE, {int((flushed & ~rne).sum())} "
          f"flushed to a signed zero instead")
    assert (rne | flushed).all()


def test_bf16_to_f32_all_patterns():
    """Every one of the 65536 bf16 bit patterns widens to the same fp32 bits as torch's conversion (NaNs: isnan)."""
    from nps_hip import ops
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    want = x.float()
    got = ops.to_f32(x.to(DEV)).cpu()
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


# ------------------------------------------------------------------ W-pass analysis
@pytest.mark.parametrize("B,H,W,m2,chans", [
    (2, 5, 24, 12, (64, 4)),     # C5's kind: two sources
    (1, 3, 33, 17, (7,)),        # odd W, m2 = W // 2 + 1 in two 16-bin chunks, scalar channel count
    (1, 2, 16, 9, (8, 3, 5)),    # m2 = W / 2 + 1 with the Nyquist bin, three sources
    (1, 2, 40, 4, (300,)),       # channels past one 256-thread pass
])
def test_spectral_dft_w_bf16_vs_fp64(B, H, W, m2, chans):
    """X1[b][h][k][c] = sum_w x[b][h][w][c] e^{-2 pi i k w / W}, k < m2: bf16 sources, fp32 spectrum."""
    from nps_hip import lib, ops, ptr, stream_ptr, check
    g = torch.Generator().manual_seed(W * 100 + m2)
    srcs = [torch.randn(B, H, W, c, generator=g).to(torch.bfloat16) for c in chans]
    C = sum(chans)
    ref = torch.fft.fft(torch.cat(srcs, dim=-1).double(), dim=2)[:, :, :m2]
    sd = [ops.Src(s.to(DEV)) for s in srcs]
    X1 = torch.full((B, H, m2, C), float("nan"), dtype=torch.complex64, device=DEV)
    check(lib.nps_spectral_dft_w_bf16(ops._c_src_bf16(sd), len(sd), B, H, W, C, m2, ptr(X1), stream_ptr()),
          "spectral_dft_w_bf16")
    err = rel_l2(X1, ref)
    print(f"spectral_dft_w_bf16 B={B} H={H} W={W} m2={m2} C={chans}: rel-L2 {err:.3e}")
    assert err < 1e-5


# ------------------------------------------------------------------ W-pass synthesis
@pytest.mark.parametrize("B,H,W,m2,Cout,fused", [
    (2, 5, 24, 12, 64, False),   # C5's kind: one chunk, plain
    (1, 3, 16, 9, 12, True),     # Nyquist; accumulate onto a bf16 out + bf16 addend + GELU
    (1, 2, 33, 17, 7, False),    # two chunks, odd W
    (1, 2, 40, 20, 68, False),   # two chunks
])
def test_spectral_idft_w_bf16_vs_fp64(B, H, W, m2, Cout, fused):
    """out = act(c2r(Z) / (H W) [+ out] [+ addend]) stored as bf16, element by element.  With r the fp64 reference
    and delta = 1e-5 rms(r) (the project's fp32 bar as absolute slack):
      m2 <= 16 (one 16-bin chunk): |y - r| <= 2^-8 |r| + delta — one round-to-nearest-even of the fp32 result
        (truncation would reach 2^-7);
      16 < m2 <= 32: |y - r| <= 2^-8 (|r| + |p1|) + delta with p1 the partial sum over the first 16 bins, which the
        kernel keeps in the bf16 output between its two chunks (include/nps.h)."""
    from nps_hip import lib, ptr, stream_ptr, check
    g = torch.Generator().manual_seed(W * 100 + m2)
    Z = torch.complex(torch.randn(B, H, m2, Cout, generator=g), torch.randn(B, H, m2, Cout, generator=g)) * (H * W / 4)
    assert (Z.imag[:, :, 0] != 0).all() and (2 * (m2 - 1) != W or (Z.imag[:, :, m2 - 1] != 0).all())
    scale = 1.0 / (H * W)
    r = _c2r_partial(Z, W, 0, m2, scale)
    out = torch.full((B, H, W, Cout), float("nan")).to(torch.bfloat16)
    addend = None
    if fused:
        out = torch.randn(B, H, W, Cout, generator=g).to(torch.bfloat16)
        addend = torch.randn(B, H, W, Cout, generator=g).to(torch.bfloat16)
        r = torch.nn.functional.gelu(r + out.double() + addend.double())
    slack = 2.0 ** -8 * r.abs() + 1e-5 * r.square().mean().sqrt()
    nchunks = (m2 + 15) // 16
    assert nchunks <= 2
    if nchunks == 2:
        slack = slack + 2.0 ** -8 * _c2r_partial(Z, W, 0, 16, scale).abs()
    Zd, outd = Z.to(DEV), out.to(DEV)
    addd = None if addend is None else addend.to(DEV)
    check(lib.nps_spectral_idft_w_bf16(ptr(Zd), ptr(outd), B, H, W, m2, Cout, 1 if fused else 0, ptr(addd),
                                       1 if fused else 0, stream_ptr()), "spectral_idft_w_bf16")
    y = outd.cpu().double()
    over = ((y - r).abs() / slack).max().item()
    print(f"spectral_idft_w_bf16 B={B} H={H} W={W} m2={m2} Cout={Cout} fused={fused}: rel-L2 {rel_l2(y, r):.3e}, "
          f"max |y - r| / bound {over:.3f}")
    assert over <= 1.0
