"""Forward nps_spectral_mix / nps_spectral_mix_bf16 over the batch, against the fp64 per-mode contraction
y[b][m][o] = sum_i x[b][m][i] W[m][i][o] (proc_fno.py:253-255).

mix_mfma_kernel has three batch regimes (16 rows per pass for B <= 16, 32 for B <= 32, several passes above), a
32-input-channel weight chunk and a 64-output-channel work-group; Cout % 4 != 0 takes the VALU kernel, which walks
the batch 8 rows at a time.  The cases put B, Cin and Cout on both sides of each of those sizes.  Y sits between
two NaN guard rows, so a store outside [0, B) x modes x [0, Cout) shows.
"""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, R, m2, Cin, Cout)
MFMA_CASES = [(1, 2, 3, 20, 12), (16, 2, 2, 32, 64), (17, 2, 2, 67, 44), (32, 1, 3, 196, 192), (33, 2, 1, 40, 68),
              (70, 1, 2, 36, 128)]
VALU_CASES = [(5, 2, 2, 20, 6), (19, 1, 3, 33, 70)]  # Cout % 4 != 0 (fp32 weights only)


def _operands(B, R, m2, Cin, Cout):
    g = torch.Generator().manual_seed(B * 1000 + Cin)

    def crand(*sh):
        return torch.complex(torch.randn(*sh, generator=g), torch.randn(*sh, generator=g))

    return crand(B, R * m2, Cin), crand(R * m2, Cin, Cout)


def _run(fn, what, X, Wd, B, R, m2, Cin, Cout):
    """Y (B, modes, Cout) of the C entry point fn, after checking the NaN guard rows on either side of it."""
    from nps_hip import ptr, stream_ptr, check
    buf = torch.view_as_complex(torch.full((B + 2, R * m2, Cout, 2), float("nan"), device=DEV))  # NaN in re and im
    Xd = X.to(DEV)
    check(fn(ptr(Xd), ptr(Wd), ptr(buf[1:B + 1]), B, R, m2, Cin, Cout, stream_ptr()), what)
    out = buf.cpu()
    assert torch.view_as_real(out[0]).isnan().all() and torch.view_as_real(out[B + 1]).isnan().all(), \
        f"{what}: wrote outside Y"
    return out[1:B + 1]


@pytest.mark.parametrize("B,R,m2,Cin,Cout", MFMA_CASES + VALU_CASES)
def test_spectral_mix_forward_vs_fp64(B, R, m2, Cin, Cout):
    from nps_hip import lib
    X, W = _operands(B, R, m2, Cin, Cout)
    ref = torch.einsum("bmi,mio->bmo", X.to(torch.complex128), W.to(torch.complex128))
    Y = _run(lib.nps_spectral_mix, "spectral_mix", X, W.to(DEV), B, R, m2, Cin, Cout)
    err = rel_l2(Y, ref)
    print(f"spectral_mix fwd B={B} R={R} m2={m2} Cin={Cin} Cout={Cout}: rel-L2 {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("B,R,m2,Cin,Cout", MFMA_CASES)
def test_spectral_mix_bf16_forward_vs_fp64(B, R, m2, Cin, Cout):
    """fp32 X2, weights rounded to bf16 (re, im) pairs by nps_f32_to_bf16; the reference contracts the same rounded
    weights in fp64, so only the fp32 arithmetic separates them."""
    from nps_hip import lib, ops
    X, W = _operands(B, R, m2, Cin, Cout)
    Wp = ops.to_bf16(W.to(DEV))                                     # (modes, Cin, Cout, 2) bf16
    Wr = torch.view_as_real(W).to(torch.bfloat16)
    assert torch.equal(Wp.cpu().view(torch.int16), Wr.view(torch.int16))
    ref = torch.einsum("bmi,mio->bmo", X.to(torch.complex128), torch.view_as_complex(Wr.double()))
    Y = _run(lib.nps_spectral_mix_bf16, "spectral_mix_bf16", X, Wp, B, R, m2, Cin, Cout)
    err = rel_l2(Y, ref)
    print(f"spectral_mix_bf16 fwd B={B} R={R} m2={m2} Cin={Cin} Cout={Cout}: rel-L2 {err:.3e}")
    assert err < 1e-5
