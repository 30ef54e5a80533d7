"""fp64 restatement of the 1-D conv entries (include/nps.h nps_conv1d_fwd / nps_conv1d_wgrad): the forward's
semantics — sources at offsets in a virtual frame, zero extension, taps, stride, out_os / out_off, accumulate, addend,
GELU — and its two gradients, written with index arithmetic and einsum only (no torch conv), on channels-last
(B, L, C) tensors.  tests/test_conv1d_ref_host.py checks it against F.conv1d / F.conv_transpose1d and
torch.autograd; the GPU tests compare the kernels with it."""
import math

import torch


def frame(srcs, L):
    """The virtual frame (B, L, sum C) in fp64: source (t, off) placed at position off (crop_Nd: > 0 zero-pads, < 0
    crops), zero outside itself and outside [0, L)."""
    cols = []
    for t, off in srcs:
        B, Ls, C = t.shape
        f = torch.zeros(B, L, C, dtype=torch.float64)
        lo, hi = max(0, off), min(L, off + Ls)
        if hi > lo:
            f[:, lo:hi] = t[:, lo - off:hi - off].double()
        cols.append(f)
    return torch.cat(cols, 2)


def out_len(L, K, stride, pad):
    return (L + pad[0] + pad[1] - K) // stride + 1


def conv(x, w, K, stride, pad):
    """y[b][l][co] = sum_{t, ci} w[co][ci][t] x[b][l*stride + t - pad_l][ci] (x zero outside itself), l < out_len."""
    B, L, _ = x.shape
    Lout = out_len(L, K, stride, pad)
    need = (Lout - 1) * stride + K
    xp = torch.zeros(B, max(need, pad[0] + L), x.shape[2], dtype=torch.float64)
    xp[:, pad[0]:pad[0] + L] = x.double()
    y = torch.zeros(B, Lout, w.shape[0], dtype=torch.float64)
    for t in range(K):
        y += torch.einsum("blc,oc->blo", xp[:, t:t + (Lout - 1) * stride + 1:stride], w[:, :, t].double())
    return y


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def conv1d_fwd(srcs, L, w, bias, stride=1, pad=(0, 0), out=None, out_os=1, out_off=0, accumulate=False, addend=None,
               act=0):
    """The forward entry.  w (Cout, Cin, K).  Returns the fp64 out (B, out_L, out_C): a given `out` is copied and
    written at rows l*out_os + out_off (rows outside it dropped, channels >= Cout untouched)."""
    K, Cout = w.shape[2], w.shape[0]
    y = conv(frame(srcs, L), w, K, stride, pad)
    if bias is not None:
        y = y + bias.double()
    res = torch.zeros(y.shape, dtype=torch.float64) if out is None else out.double().clone()
    for l in range(y.shape[1]):
        ol = l * out_os + out_off
        if not 0 <= ol < res.shape[1]:
            continue
        v = y[:, l]
        if addend is not None:
            v = v + addend[:, ol, :Cout].double()
        if act == 1:
            v = gelu(v)
        res[:, ol, :Cout] = res[:, ol, :Cout] + v if accumulate else v
    return res


def written_rows(Lout, out_L, out_os, out_off):
    return [l * out_os + out_off for l in range(Lout) if 0 <= l * out_os + out_off < out_L]


def conv1d_dx(dy, w, L, stride, pad):
    """dL/dx (B, L, Cin) of y = conv(x, w): dx[b][i][ci] = sum over l*stride + t - pad_l = i of dy[b][l][co] w[co][ci][t]."""
    B, Ly, _ = dy.shape
    dx = torch.zeros(B, L, w.shape[1], dtype=torch.float64)
    for l in range(Ly):
        for t in range(w.shape[2]):
            i = l * stride + t - pad[0]
            if 0 <= i < L:
                dx[:, i] += dy[:, l].double() @ w[:, :, t].double()
    return dx


def conv1d_dw(a, x, K, stride, pad):
    """The weight-gradient entry: g[m][n][t] = sum_{b,l} a[b][l][m] xz[b][l*stride + t - pad_l][n]."""
    B, La, M = a.shape
    Lx = x.shape[1]
    g = torch.zeros(M, x.shape[2], K, dtype=torch.float64)
    for t in range(K):
        for l in range(La):
            i = l * stride + t - pad[0]
            if 0 <= i < Lx:
                g[:, :, t] += a[:, l].double().t() @ x[:, i].double()
    return g


def conv_transpose1d(x, w, bias, p):
    """nn.ConvTranspose1d(k=4, s=2, padding=p) on channels-last x (B, L, Cin), w (Cin, Cout, 4): the two 2-tap phases
    of the forward entry, out_os = 2 (how the HIP path runs it)."""
    B, L, _ = x.shape
    out = torch.zeros(B, 2 * L + 2 - 2 * p, w.shape[1], dtype=torch.float64)
    for r in (0, 1):
        out = conv1d_fwd([(x, 0)], L, phase_weight(w, r), bias, pad=(1, 1), out=out, out_os=2, out_off=r - p)
    return out


def phase_weight(w, r):
    """W_r[co][ci][t] = w[ci][co][2 (1 - t) + r] of a k4/s2 transposed conv weight w (Cin, Cout, 4)."""
    wt = w.transpose(0, 1)
    return torch.stack((wt[:, :, 2 + r], wt[:, :, r]), 2)


def rand(shape, seed):
    """Uniform in [-1, 1], fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1
