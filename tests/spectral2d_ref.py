"""fp64 restatement of the SpectralConv2d stages in the layouts of include/nps.h ("SpectralConv2d forward", and the
3-D weight packing of "SpectralConv3d"), written from their formulas as explicit cos / sin matrices and einsum — no
torch.fft — so that each function is the definition of its stage, and differentiable by torch autograd (complex
tensors: PyTorch's conj convention).  The backward stages have no formula of their own here: they are autograd
through these functions.

test_spectral2d_ref_host.py pins the composition to the module formula irfft2(P(rfft2(x))) and the 3-D pack to the
reference's four corner writes; test_gpu_spectral_stages.py uses the functions one stage at a time.
"""
import math

import torch


def k1_rows(H, m1):
    """Frequency of each retained row: rows [:m1] and [-m1:] of an H-point axis, R = min(H, 2 m1) distinct ones."""
    R = min(H, 2 * m1)
    return [r if r < m1 else H - R + r for r in range(R)]


def twiddles(N, ks):
    """cos, sin (len(ks), N) fp64 of 2 pi (k n mod N) / N."""
    k = torch.as_tensor(list(ks), dtype=torch.int64)[:, None]
    n = torch.arange(N, dtype=torch.int64)[None, :]
    ph = ((k * n) % N).double() * (2.0 * math.pi / N)
    return torch.cos(ph), torch.sin(ph)


def _c128(t):
    return t.to(torch.complex128)


def dft_w(x, m2):
    """X1 (B, H, m2, C) complex128 = sum_w x[b][h][w][c] e^{-2 pi i k w / W} for real x (B, H, W, C)."""
    cos, sin = twiddles(x.shape[2], range(m2))
    xd = x.double()
    return torch.complex(torch.einsum("bhwc,kw->bhkc", xd, cos), -torch.einsum("bhwc,kw->bhkc", xd, sin))


def dft_h(X1, m1):
    """X2 (B, R, m2, C) = sum_h X1[b][h][k][c] e^{-2 pi i k1(r) h / H}."""
    X1 = _c128(X1)
    cos, sin = twiddles(X1.shape[1], k1_rows(X1.shape[1], m1))
    re = torch.einsum("bhkc,rh->brkc", X1.real, cos) + torch.einsum("bhkc,rh->brkc", X1.imag, sin)
    im = torch.einsum("bhkc,rh->brkc", X1.imag, cos) - torch.einsum("bhkc,rh->brkc", X1.real, sin)
    return torch.complex(re, im)


def pack(w1, w2, H):
    """wpack (R, m2, Cin, Cout) from weights1 / weights2 (Cin, Cout, m1, m2), in their dtype: the reference writes
    rows [:m1] from weights1, then rows [-m1:] from weights2, so a row both corners cover holds weights2."""
    m1 = w1.shape[2]
    dense = torch.zeros((H, w1.shape[3], w1.shape[0], w1.shape[1]), dtype=w1.dtype)
    dense[:m1] = w1.permute(2, 3, 0, 1)
    dense[H - m1:] = w2.permute(2, 3, 0, 1)
    return dense[k1_rows(H, m1)]


def mix(X2, wpack):
    """Y (B, R, m2, Cout) = sum_i X2[b][r][k][i] wpack[r][k][i][o] (the plain einsum mixer)."""
    return torch.einsum("brki,rkio->brko", _c128(X2), _c128(wpack))


def idft_h(Y, H, m1):
    """Z (B, H, m2, Cout) = sum_r Y[b][r][k][o] e^{+2 pi i k1(r) h / H}."""
    Y = _c128(Y)
    cos, sin = twiddles(H, k1_rows(H, m1))
    re = torch.einsum("brko,rh->bhko", Y.real, cos) - torch.einsum("brko,rh->bhko", Y.imag, sin)
    im = torch.einsum("brko,rh->bhko", Y.real, sin) + torch.einsum("brko,rh->bhko", Y.imag, cos)
    return torch.complex(re, im)


def c2r_partial(Z, W, k0, k1, scale, doubling=True):
    """scale * sum_{k0 <= k < k1} c_k Re(Z[..., k, :] e^{2 pi i k w / W}) -> (B, H, W, Cout) fp64: the one-sided c2r
    synthesis (DC and, for even W, Nyquist once with their imaginary parts dropped; every other bin twice).
    doubling=False counts every bin once (the adjoint of dft_w)."""
    k = torch.arange(k0, k1, dtype=torch.float64)
    self_conj = (k == 0) | (2 * k == W)
    ck = 2.0 - self_conj.double() if doubling else torch.ones_like(k)
    ang = 2 * math.pi * k[:, None] * torch.arange(W, dtype=torch.float64)[None, :] / W      # (k, w)
    Zr, Zi = Z.real.double()[:, :, k0:k1], Z.imag.double()[:, :, k0:k1]
    Zi = Zi * (~self_conj).double()[None, None, :, None]
    return scale * (torch.einsum("bhko,kw->bhwo", Zr, ck[:, None] * torch.cos(ang)) -
                    torch.einsum("bhko,kw->bhwo", Zi, ck[:, None] * torch.sin(ang)))


def idft_w(Z, W, scale, doubling=True):
    """y (B, H, W, Cout) fp64 = scale * c2r_W(Z) over all the bins of Z (B, H, m2, Cout)."""
    return c2r_partial(Z, W, 0, Z.shape[2], scale, doubling)


def spectral2d(x, w1, w2):
    """SpectralConv2d on NHWC x (B, H, W, Cin): the stages composed, fp64."""
    H, W = x.shape[1], x.shape[2]
    m1, m2 = w1.shape[2], w1.shape[3]
    Y = mix(dft_h(dft_w(x, m2), m1), pack(w1, w2, H))
    return idft_w(idft_h(Y, H, m1), W, 1.0 / (H * W))


def pack3d(w1, w2, w3, w4, D, H):
    """wpack (R1, R2, m3, Cin, Cout) from weights1..4 (Cin, Cout, m1, m2, m3), in their dtype.  The reference writes
    the corners [:m1, :m2], [-m1:, :m2], [:m1, -m2:], [-m1:, -m2:] in this order: a later write owns the mode."""
    m1, m2 = w1.shape[2], w1.shape[3]
    dense = torch.zeros((D, H, w1.shape[4], w1.shape[0], w1.shape[1]), dtype=w1.dtype)
    dense[:m1, :m2] = w1.permute(2, 3, 4, 0, 1)
    dense[D - m1:, :m2] = w2.permute(2, 3, 4, 0, 1)
    dense[:m1, H - m2:] = w3.permute(2, 3, 4, 0, 1)
    dense[D - m1:, H - m2:] = w4.permute(2, 3, 4, 0, 1)
    return dense[k1_rows(D, m1)][:, k1_rows(H, m2)]
