"""Stage-by-stage checks of the fp32 channels-last SpectralConv2d kernels of csrc/spectral.hip (and the 3-D weight
packing of csrc/spectral3d.hip) against the fp64 restatement tests/spectral2d_ref.py: the two analysis passes, the two
synthesis passes with their epilogues and range tag, the two adjoint W passes (reference: torch fp64 autograd through
the restatement) and the pack / unpack pairs (copies: bit for bit).

Every case is the smallest shape that selects one dispatch path of launch_dft_w / nps_spectral_dft_h /
nps_spectral_idft_h / launch_idft_w, and carries that selector as a comment.  Inputs are N(0, 1) from a seeded
generator.  Each output lies NaN-filled inside a larger buffer with one guard row (the innermost C elements) of a
sentinel bit pattern before and after it, which must come back untouched.  Bar: the project's fp32 rel-L2 < 1e-5
against fp64, on the whole tensor and on every slice along the transformed axis of the output (bin k of a W analysis,
retained row r of the H analysis, row h of the H synthesis, pixel w of a W synthesis), so that one wrong bin or row
cannot hide in the norm of the others.  Measured values: profiles/spectral_stages/README.md.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
import spectral2d_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
SENTINEL = 0x7FA5C3B1   # a NaN payload that no kernel produces (the fill of the output itself is the default NaN)


# ------------------------------------------------------------------ helpers
def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _crandn(g, *shape):
    return torch.complex(_randn(g, *shape), _randn(g, *shape))


class Guarded:
    """An fp32 / complex64 device tensor of `shape`, NaN-filled, between two guard rows of SENTINEL words."""

    def __init__(self, shape, complex_=False):
        per = 2 if complex_ else 1
        n = per * int(torch.tensor(shape).prod())
        self.row = per * shape[-1]
        self.buf = torch.empty(n + 2 * self.row, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(SENTINEL)
        body = self.buf[self.row:self.row + n]
        body.fill_(float("nan"))
        self.t = torch.view_as_complex(body.view(*shape, 2)) if complex_ else body.view(*shape)

    def assert_guards(self):
        torch.cuda.synchronize()
        words = self.buf.view(torch.int32)
        assert (words[:self.row] == SENTINEL).all(), "the guard row before the output was written"
        assert (words[-self.row:] == SENTINEL).all(), "the guard row after the output was written"


def _same_bits(a, b):
    f = lambda t: (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)
    return torch.equal(f(a), f(b))


def _check(what, got, ref, dim, tol=TOL):
    """Whole-tensor rel-L2 and the same bar on every slice along `dim` of the output; prints the measured values."""
    got, ref = got.detach().cpu(), ref.detach()
    whole = rel_l2(got, ref)
    n = ref.shape[dim]
    rms = [ref.select(dim, i).abs().square().mean().sqrt().item() for i in range(n)]
    # N(0, 1) inputs: no slice of the reference is near zero, so a relative error per slice is meaningful
    assert min(rms) > 0.1 * ref.abs().square().mean().sqrt().item(), (what, rms)
    per = [rel_l2(got.select(dim, i), ref.select(dim, i)) for i in range(n)]
    worst = max(range(n), key=lambda i: per[i] if per[i] == per[i] else float("inf"))
    print(f"{what}: rel-L2 {whole:.3e}, worst slice (dim {dim}, index {worst}) {per[worst]:.3e}")
    assert whole < tol, what
    bad = [(i, e) for i, e in enumerate(per) if not e < tol]
    assert not bad, (what, bad)


def _api():
    from nps_hip import lib, ops, ptr, stream_ptr, check
    return lib, ops, ptr, stream_ptr, check


# ------------------------------------------------------------------ nps_spectral_dft_w
def _run_dft_w(srcs, m2):
    lib, ops, ptr, stream_ptr, check = _api()
    B, H, W = srcs[0].shape[:3]
    C = sum(s.shape[3] for s in srcs)
    sd = [ops.Src(s.to(DEV)) for s in srcs]
    X1 = Guarded((B, H, m2, C), complex_=True)
    check(lib.nps_spectral_dft_w(ops._c_src(sd), len(sd), B, H, W, C, m2, ptr(X1.t), stream_ptr()), "spectral_dft_w")
    X1.assert_guards()
    return X1.t


def _hbig():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return -(-(8 * cus + 40) // 3)


DFT_W_CASES = [
    # B, H, W, m2, source channel counts.  MFMA: every source C % 4 == 0, m2 <= 16, even W (launch_dft_w)
    (2, 3, 16, 9, (8,)),           # MFMA, Nyquist bin k = 8, W exactly one 16-pixel batch
    (1, 2, 30, 16, (12,)),         # MFMA, all 16 cos / sin rows live, Nyquist at k = 15, tail of 7 K-steps
    (1, 2, 34, 16, (8,)),          # MFMA, bin k = 15 below Nyquist: all 16 sin rows nonzero, tail of 1 K-step
    (1, 2, 22, 5, (132,)),         # MFMA, two 128-channel groups, the second holding 4 channels
    (1, 3, 20, 6, (4, 124, 8)),    # MFMA, source boundaries inside and across 128-channel groups
    (3, "Hbig", 6, 4, (4, 4)),     # MFMA persistent loop: rows x groups > 8 x CUs, 40 waves take a second task
    (1, 3, 17, 9, (8,)),           # odd W -> VALU KC = 12 with three zero bins, pixel tail of 1
    (1, 2, 16, 3, (7,)),           # VALU KC = 4, unaligned source
    (1, 2, 24, 7, (5, 3)),         # VALU KC = 8, two unaligned sources
    (1, 2, 30, 16, (70,)),         # VALU KC = 16 with all 16 bins live (W >= 30 for 16 bins), block size 128
    (1, 2, 40, 21, (8,)),          # aligned and even W, but m2 > 16 -> VALU, two chunks
    (1, 2, 12, 4, (300,)),         # channels past one 256-thread pass
]


@pytest.mark.parametrize("B,H,W,m2,chans", DFT_W_CASES)
def test_dft_w_vs_fp64(B, H, W, m2, chans):
    """X1[b][h][k][c] = sum_w x[b][h][w][c] e^{-2 pi i k w / W}, k < m2."""
    H = _hbig() if H == "Hbig" else H
    g = torch.Generator().manual_seed(1000 * W + 10 * m2 + len(chans))
    srcs = [_randn(g, B, H, W, c) for c in chans]
    got = _run_dft_w(srcs, m2)
    _check(f"dft_w B={B} H={H} W={W} m2={m2} C={chans}", got, R.dft_w(torch.cat(srcs, dim=-1), m2), dim=2)


@pytest.mark.parametrize("B,H,W,m2,split", [
    (1, 2, 22, 5, (60, 72)),   # MFMA on both sides (132 channels), the boundary inside the first 128-channel group
    (1, 2, 24, 7, (5, 2)),     # VALU on both sides (7 channels: no 4-aligned source on either)
])
def test_dft_w_sources_and_repeat_bit_exact(B, H, W, m2, split):
    """Two sources give the bits of their concatenation as one source, and a second run repeats the first."""
    g = torch.Generator().manual_seed(W)
    x = _randn(g, B, H, W, sum(split))
    one = _run_dft_w([x], m2)
    two = _run_dft_w([t.contiguous() for t in x.split(list(split), dim=-1)], m2)
    assert not one.isnan().any()
    assert _same_bits(one, two)
    assert _same_bits(one, _run_dft_w([x], m2))


def test_dft_w_refuses_bins_past_nyquist():
    """m2 = 16 of a 24-pixel row (13 bins exist): an error code, nothing written."""
    lib, ops, ptr, stream_ptr, check = _api()
    x = ops.Src(torch.randn(1, 2, 24, 70).to(DEV))
    X1 = Guarded((1, 2, 16, 70), complex_=True)
    rc = lib.nps_spectral_dft_w(ops._c_src([x]), 1, 1, 2, 24, 70, 16, ptr(X1.t), stream_ptr())
    assert rc != 0 and "m2=16 W=24" in lib.nps_last_error().decode()
    X1.assert_guards()
    assert torch.view_as_real(X1.t).isnan().all()


# ------------------------------------------------------------------ nps_spectral_dft_h / nps_spectral_idft_h
H_CASES = [
    # B, H, m1, m2, C.  R = min(H, 2 m1) retained rows, RC = R rounded up to 8 / 16 / 24 / 32, NC = m2 C columns
    (2, 6, 4, 3, 5),        # overlapping corners, R = H = 6, RC 8
    (1, 1, 1, 2, 3),        # H = m1 = 1
    (1, 5, 5, 1, 4),        # H = m1
    (1, 21, 5, 3, 23),      # RC 16 with 10 live rows, H % 16 != 0, NC = 69
    (2, 37, 9, 2, 8),       # RC 24, 18 live rows
    (1, 33, 13, 2, 4),      # RC 32, 26 live rows
    (1, 32, 16, 1, 70),     # RC 32, 32 live rows
    (1, 400, 13, 1, 3),     # dft_h: RC 32 table over 96 KiB -> generic kernel
    (1, 520, 8, 1, 3),      # dft_h: RC 16 table between 64 and 96 KiB of dynamic LDS
    (1, 1030, 4, 1, 2),     # dft_h: RC 8 table between 64 and 96 KiB of dynamic LDS
    (6, 5, 2, 8, 4),        # a 3-D call: B D batches with m2 := R2 m3
]


@pytest.mark.parametrize("B,H,m1,m2,C", H_CASES + [
    (1, 40, 17, 3, 100),    # R = 34 -> generic kernel, five row chunks, the last with 2 rows, NC = 300
])
def test_dft_h_vs_fp64(B, H, m1, m2, C):
    """X2[b][r][k][c] = sum_h X1[b][h][k][c] e^{-2 pi i k1(r) h / H}."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * H + 10 * m1 + C)
    X1 = _crandn(g, B, H, m2, C)
    X2, X1d = Guarded((B, min(H, 2 * m1), m2, C), complex_=True), X1.to(DEV)
    check(lib.nps_spectral_dft_h(ptr(X1d), ptr(X2.t), B, H, m1, m2, C, stream_ptr()), "spectral_dft_h")
    X2.assert_guards()
    _check(f"dft_h B={B} H={H} m1={m1} m2={m2} C={C}", X2.t, R.dft_h(X1, m1), dim=1)


@pytest.mark.parametrize("B,H,m1,m2,C", H_CASES + [
    (1, 2, 1, 2, 3),        # fewer rows than waves
    (1, 3, 2, 1, 4),        # fewer rows than waves, overlapping corners
    (1, 70, 6, 1, 69),      # two 64-row blocks, the last with 6 rows; NC % 64 != 0
])
def test_idft_h_vs_fp64(B, H, m1, m2, C):
    """Z[b][h][k][o] = sum_r Y[b][r][k][o] e^{+2 pi i k1(r) h / H}."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * H + 10 * m1 + C + 1)
    Y = _crandn(g, B, min(H, 2 * m1), m2, C)
    Z, Yd = Guarded((B, H, m2, C), complex_=True), Y.to(DEV)
    check(lib.nps_spectral_idft_h(ptr(Yd), ptr(Z.t), B, H, m1, m2, C, stream_ptr()), "spectral_idft_h")
    Z.assert_guards()
    _check(f"idft_h B={B} H={H} m1={m1} m2={m2} C={C}", Z.t, R.idft_h(Y, H, m1), dim=1)


def test_idft_h_refuses_more_than_32_rows():
    """R = 34 retained rows: an error code and a message naming them, nothing written."""
    lib, ops, ptr, stream_ptr, check = _api()
    B, H, m1, m2, C = 1, 40, 17, 1, 4
    Y = _crandn(torch.Generator().manual_seed(0), B, 34, m2, C).to(DEV)
    Z = Guarded((B, H, m2, C), complex_=True)
    rc = lib.nps_spectral_idft_h(ptr(Y), ptr(Z.t), B, H, m1, m2, C, stream_ptr())
    msg = lib.nps_last_error().decode()
    assert rc != 0 and "34 retained rows" in msg, (rc, msg)
    Z.assert_guards()
    assert torch.view_as_real(Z.t).isnan().all()


# ------------------------------------------------------------------ nps_spectral_idft_w
IDFT_W_CASES = [
    # B, H, W, m2, Cout
    (1, 2, 16, 3, 7),       # KC = 4
    (2, 3, 16, 9, 12),      # KC = 12, Nyquist
    (1, 2, 17, 8, 5),       # odd W, KC = 8
    (1, 2, 40, 16, 68),     # KC = 16
    (1, 2, 32, 17, 6),      # two chunks, Nyquist in the second chunk
    (1, 2, 64, 33, 5),      # three chunks: one that is neither first nor last
    (1, 2, 20, 5, 300),     # two passes over Cout
]


def _spectrum(g, B, H, W, m2, C, amp=1.0):
    """Z with nonzero imaginary parts at DC and (where retained) Nyquist, which the synthesis must drop."""
    Z = _crandn(g, B, H, m2, C) * amp
    assert (Z.imag[:, :, 0] != 0).all() and (2 * (m2 - 1) != W or (Z.imag[:, :, m2 - 1] != 0).all())
    return Z


@pytest.mark.parametrize("B,H,W,m2,Cout", IDFT_W_CASES)
def test_idft_w_vs_fp64(B, H, W, m2, Cout):
    """out = c2r_W(Z) / (H W): DC and Nyquist once without their imaginary parts, every other bin twice."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * W + 10 * m2 + Cout)
    Z = _spectrum(g, B, H, W, m2, Cout)
    out, Zd = Guarded((B, H, W, Cout)), Z.to(DEV)
    check(lib.nps_spectral_idft_w(ptr(Zd), ptr(out.t), B, H, W, m2, Cout, 0, None, 0, None, stream_ptr()),
          "spectral_idft_w")
    out.assert_guards()
    _check(f"idft_w B={B} H={H} W={W} m2={m2} Cout={Cout}", out.t, R.idft_w(Z, W, 1.0 / (H * W)), dim=2)


@pytest.mark.parametrize("epilogue", ["plain", "accumulate", "addend", "accumulate+addend+gelu"])
@pytest.mark.parametrize("B,H,W,m2,Cout", [
    (2, 3, 16, 9, 12),      # one chunk
    (1, 2, 32, 17, 6),      # two chunks: the first must not see addend / GELU, the second reads its partial sum
])
def test_idft_w_epilogues_vs_fp64(B, H, W, m2, Cout, epilogue):
    """out = act(c2r_W(Z) / (H W) [+ out] [+ addend]).  Z is scaled by H W / 4, so that the synthesis is of the
    size of the N(0, 1) out / addend it is added to and its error shows in the sum."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * W + 10 * m2 + Cout)
    Z = _spectrum(g, B, H, W, m2, Cout, amp=H * W / 4)
    out0, addend = _randn(g, B, H, W, Cout), _randn(g, B, H, W, Cout)
    acc, add, act = "accumulate" in epilogue, "addend" in epilogue, "gelu" in epilogue
    ref = R.idft_w(Z, W, 1.0 / (H * W))
    out = Guarded((B, H, W, Cout))
    if acc:
        out.t.copy_(out0)
        ref = ref + out0.double()
    if add:
        ref = ref + addend.double()
    if act:
        ref = F.gelu(ref)
    Zd, addd = Z.to(DEV), addend.to(DEV)
    check(lib.nps_spectral_idft_w(ptr(Zd), ptr(out.t), B, H, W, m2, Cout, int(acc), ptr(addd) if add else None,
                                  int(act), None, stream_ptr()),
          "spectral_idft_w")
    out.assert_guards()
    _check(f"idft_w {epilogue} B={B} H={H} W={W} m2={m2} Cout={Cout}", out.t, ref, dim=2)


@pytest.mark.parametrize("B,H,W,m2,Cout", [(2, 3, 16, 9, 12), (1, 2, 32, 17, 6)])
def test_idft_w_range_tag_is_the_output_max(B, H, W, m2, Cout):
    """Through the NhwcW adapter on a fresh tensor: the tag the kernel raises is max |out| exactly."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(W + m2)
    Z = _spectrum(g, B, H, W, m2, Cout)
    out = Guarded((B, H, W, Cout))
    Zd = Z.to(DEV)
    ops.NhwcW([ops.Src(torch.empty(B, H, W, 1, device=DEV))]).idft_w(Zd, out.t, m2, Cout)
    out.assert_guards()
    assert ops.tag_value(out.t) == float(out.t.abs().max())
    assert rel_l2(out.t, R.idft_w(Z, W, 1.0 / (H * W))) < TOL


def test_idft_w_range_tag_ignores_an_intermediate_chunk():
    """Two chunks whose first partial sum is far larger than the result: the first 16 bins carry 8x the amplitude of
    the 17th and `addend` is minus their (fp32-rounded) partial sum, so the final values are the small remainder.
    The tag bounds what the kernel wrote last, so it must equal the max of the output, not of the partial sum.  The
    sum cancels by construction: values are compared with the absolute slack 1e-5 rms(|partial| + |rest| + |addend|),
    the fp32 bar on the magnitudes that were actually added."""
    lib, ops, ptr, stream_ptr, check = _api()
    B, H, W, m2, Cout = 1, 2, 32, 17, 6
    g = torch.Generator().manual_seed(7)
    Z = _spectrum(g, B, H, W, m2, Cout)
    Z[:, :, :16] *= 8.0
    scale = 1.0 / (H * W)
    partial = R.c2r_partial(Z, W, 0, 16, scale)
    rest = R.c2r_partial(Z, W, 16, m2, scale)
    addend = (-partial).float().contiguous()   # (einsum's result is a permuted view)
    ref = partial + rest + addend.double()
    assert partial.abs().max() > 2 * ref.abs().max()
    out = Guarded((B, H, W, Cout))
    Zd, addd = Z.to(DEV), addend.to(DEV)
    ops.NhwcW([ops.Src(torch.empty(B, H, W, 1, device=DEV))]).idft_w(Zd, out.t, m2, Cout, addend=addd)
    out.assert_guards()
    got = out.t.cpu().double()
    slack = 1e-5 * (partial.abs() + rest.abs() + addend.double().abs()).square().mean().sqrt().item()
    err = (got - ref).abs().max().item()
    tag, omax = ops.tag_value(out.t), float(out.t.abs().max())
    print(f"idft_w tag, cancelling addend: max |y - r| {err:.3e} (slack {slack:.3e}), tag {tag:.6g}, max |out| "
          f"{omax:.6g}, max |partial| {partial.abs().max().item():.6g}")
    assert err <= slack
    assert tag == omax


# ------------------------------------------------------------------ the adjoint W passes
@pytest.mark.parametrize("B,H,W,m2,Cout", [
    (2, 3, 16, 9, 8),       # MFMA with c2r_adj and the Nyquist bin
    (1, 2, 30, 16, 132),    # MFMA with c2r_adj, Nyquist at k = 15, two channel groups
    (1, 2, 34, 16, 8),      # MFMA with c2r_adj, bin k = 15 doubled (below Nyquist)
    (1, 2, 24, 5, 4),       # MFMA, no Nyquist bin retained
    (1, 2, 17, 9, 8),       # odd W: every bin but DC doubled (VALU)
    (1, 2, 16, 9, 7),       # VALU with Nyquist
    (1, 2, 32, 17, 6),      # chunked, Nyquist at kb + k in the second chunk
])
def test_idft_w_bwd_vs_fp64_autograd(B, H, W, m2, Cout):
    """gZ = d<gy, idft_w(Z)>/dZ under torch autograd (PyTorch's complex convention) through the restatement."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * W + 10 * m2 + Cout + 3)
    gy = _randn(g, B, H, W, Cout)
    Z = _crandn(g, B, H, m2, Cout).to(torch.complex128).requires_grad_()
    ref, = torch.autograd.grad(R.idft_w(Z, W, 1.0 / (H * W)), Z, gy.double())
    gZ, gyd = Guarded((B, H, m2, Cout), complex_=True), gy.to(DEV)
    check(lib.nps_spectral_idft_w_bwd(ptr(gyd), ptr(gZ.t), B, H, W, m2, Cout, stream_ptr()),
          "spectral_idft_w_bwd")
    gZ.assert_guards()
    _check(f"idft_w_bwd B={B} H={H} W={W} m2={m2} Cout={Cout}", gZ.t, ref, dim=2)


@pytest.mark.parametrize("B,H,W,m2,Cin", IDFT_W_CASES)
def test_dft_w_bwd_vs_fp64_autograd(B, H, W, m2, Cin):
    """gx = the gradient of dft_w at cotangent gX1 under torch autograd through the restatement (idft_w_kernel with
    doubling = 0, scale 1)."""
    lib, ops, ptr, stream_ptr, check = _api()
    g = torch.Generator().manual_seed(1000 * W + 10 * m2 + Cin + 5)
    gX1 = _crandn(g, B, H, m2, Cin)
    x = _randn(g, B, H, W, Cin).double().requires_grad_()
    ref, = torch.autograd.grad(R.dft_w(x, m2), x, gX1.to(torch.complex128))
    gx, gd = Guarded((B, H, W, Cin)), gX1.to(DEV)
    check(lib.nps_spectral_dft_w_bwd(ptr(gd), ptr(gx.t), B, H, W, m2, Cin, stream_ptr()),
          "spectral_dft_w_bwd")
    gx.assert_guards()
    _check(f"dft_w_bwd B={B} H={H} W={W} m2={m2} Cin={Cin}", gx.t, ref, dim=2)


# ------------------------------------------------------------------ pack / unpack: copies, bit for bit
def _pack_adjoint(pack, ws, gwp):
    """Gradients of the weights under the restated pack at cotangent gwp: gwp's values where the weight is read,
    exact zeros where a later corner overwrote it."""
    leaves = [w.clone().requires_grad_() for w in ws]
    return torch.autograd.grad(pack(*leaves), leaves, gwp)


@pytest.mark.parametrize("H,m1", [
    (10, 3),    # no overlap
    (6, 4),     # partial overlap: weights1 rows 2, 3 overwritten
    (8, 4),     # H == 2 m1: the corners meet
    (5, 5),     # H == m1: weights2 owns every row
])
def test_pack_unpack_2d_bit_exact(H, m1):
    lib, ops, ptr, stream_ptr, check = _api()
    Cin, Cout, m2 = 3, 5, 2
    Rr = min(H, 2 * m1)
    g = torch.Generator().manual_seed(10 * H + m1)
    ws = [_crandn(g, Cin, Cout, m1, m2) for _ in range(2)]
    wp = Guarded((Rr, m2, Cin, Cout), complex_=True)
    wd = [w.to(DEV) for w in ws]
    check(lib.nps_spectral_pack_weights(*[ptr(w) for w in wd], ptr(wp.t), Cin, Cout, H, m1, m2, stream_ptr()),
          "spectral_pack_weights")
    wp.assert_guards()
    assert _same_bits(wp.t.cpu(), R.pack(*ws, H))
    gwp = _crandn(g, Rr, m2, Cin, Cout)
    want = _pack_adjoint(functools.partial(R.pack, H=H), ws, gwp)
    gws, gwpd = [Guarded((Cin, Cout, m1, m2), complex_=True) for _ in range(2)], gwp.to(DEV)
    check(lib.nps_spectral_unpack_grad(ptr(gwpd), *[ptr(t.t) for t in gws], Cin, Cout, H, m1, m2,
                                       stream_ptr()), "spectral_unpack_grad")
    for i, (got, w) in enumerate(zip(gws, want)):
        got.assert_guards()
        assert _same_bits(got.t.cpu(), w), f"gweights{i + 1}"
    assert (want[0][:, :, max(H - m1, 0):] == 0).all()


@pytest.mark.parametrize("D,H,m1,m2", [
    (8, 9, 2, 3),   # no overlap
    (3, 9, 2, 3),   # overlap along D only
    (8, 4, 2, 3),   # overlap along H only
    (3, 5, 2, 3),   # overlap along both
    (2, 3, 2, 3),   # D == m1 and H == m2: weights4 owns every mode
])
def test_pack_unpack_3d_bit_exact(D, H, m1, m2):
    lib, ops, ptr, stream_ptr, check = _api()
    Cin, Cout, m3 = 3, 5, 2
    R1, R2 = min(D, 2 * m1), min(H, 2 * m2)
    g = torch.Generator().manual_seed(100 * D + H)
    ws = [_crandn(g, Cin, Cout, m1, m2, m3) for _ in range(4)]
    wp = Guarded((R1, R2, m3, Cin, Cout), complex_=True)
    wd = [w.to(DEV) for w in ws]
    check(lib.nps_spectral3d_pack_weights(*[ptr(w) for w in wd], ptr(wp.t), Cin, Cout, D, H, m1, m2, m3,
                                          stream_ptr()), "spectral3d_pack_weights")
    wp.assert_guards()
    assert _same_bits(wp.t.cpu(), R.pack3d(*ws, D, H))
    gwp = _crandn(g, R1, R2, m3, Cin, Cout)
    want = _pack_adjoint(functools.partial(R.pack3d, D=D, H=H), ws, gwp)
    gws, gwpd = [Guarded((Cin, Cout, m1, m2, m3), complex_=True) for _ in range(4)], gwp.to(DEV)
    check(lib.nps_spectral3d_unpack_grad(ptr(gwpd), *[ptr(t.t) for t in gws], Cin, Cout, D, H, m1, m2, m3,
                                         stream_ptr()), "spectral3d_unpack_grad")
    for i, (got, w) in enumerate(zip(gws, want)):
        got.assert_guards()
        assert _same_bits(got.t.cpu(), w), f"gweights{i + 1}"
