"""fp64 restatement of the SpectralConv1d / FNO-1D contract (include/nps.h, "SpectralConv1d"), written from its
formulas as explicit cos / sin matrix products — no torch.fft — and differentiable by torch autograd (complex
weights: PyTorch's conj convention, the one the fixture's gradients were recorded under).

test_spectral1d_host.py pins it to every output of the reference recorded in tests/golden/fno1d.pt; the GPU tests
use it, with autograd, as the reference at shapes the fixture does not cover.
"""
import math

import torch
import torch.nn.functional as F


def twiddles(L, m):
    """cos, sin (m, L) fp64 of 2 pi (k l mod L) / L."""
    k = torch.arange(m, dtype=torch.int64)[:, None]
    l = torch.arange(L, dtype=torch.int64)[None, :]
    ph = ((k * l) % L).double() * (2.0 * math.pi / L)
    return torch.cos(ph), torch.sin(ph)


def analysis(x, m):
    """X (B, m, C) complex128 = sum_l x[b][c][l] e^{-2 pi i k l / L} for x (B, C, L)."""
    cos, sin = twiddles(x.shape[2], m)
    xd = x.double()
    return torch.complex(torch.einsum("bcl,kl->bkc", xd, cos), -torch.einsum("bcl,kl->bkc", xd, sin))


def film_factor(p, Wf, bf, Cout, m, mode):
    """S (B, m, Cout) fp64: F = p Wf^T + bf viewed (B, Cout, m); 1 + F (mode 0) or F (mode 1)."""
    Fw = (p.double() @ Wf.double().t() + bf.double()).view(p.shape[0], Cout, m).permute(0, 2, 1)
    return 1.0 + Fw if mode == 0 else Fw


def synthesis(Y, L):
    """y (B, C, L) fp64 = (1 / L) [Re Y_0 + sum_{k >= 1} c_k (Re Y_k cos - Im Y_k sin)], c_k = 1 for the Nyquist bin
    of an even L, else 2; Im of DC and Nyquist dropped."""
    m = Y.shape[1]
    cos, sin = twiddles(L, m)
    k = torch.arange(m)
    self_conj = (k == 0) | (2 * k == L)
    c = torch.where(self_conj, 1.0, 2.0).double()[None, :, None]
    keep_im = (~self_conj).double()[None, :, None]
    return (torch.einsum("bkc,kl->bcl", Y.real * c, cos) - torch.einsum("bkc,kl->bcl", Y.imag * c * keep_im, sin)) / L


def spectral1d_ref(x, w, film=None):
    """SpectralConv1d: x (B, Cin, L), w (Cin, Cout, m) complex -> (B, Cout, L) fp64; film = (p, Wf, bf, mode)."""
    Cout, m = w.shape[1], w.shape[2]
    Y = torch.einsum("bki,iok->bko", analysis(x, m), w.to(torch.complex128))
    if film is not None:
        p, Wf, bf, mode = film
        Y = Y * film_factor(p, Wf, bf, Cout, m, mode)
    return synthesis(Y, x.shape[2])


def _conv(sd, prefix, x, p, mode):
    film = None
    if prefix + "weights_feat.weight" in sd:
        film = (p, sd[prefix + "weights_feat.weight"], sd[prefix + "weights_feat.bias"], mode)
    return spectral1d_ref(x, sd[prefix + "weights1"], film)


def fno_layer1d_ref(sd, prefix, x, p=None):
    """FNO_Layer 1-D (pointwise w [+ w2], GELU) with its default transform_mode 0, fp64."""
    y = _conv(sd, prefix + "conv.", x, p, 0)
    y = y + F.conv1d(x.double(), sd[prefix + "w.weight"].double(), sd[prefix + "w.bias"].double())
    if prefix + "w2.weight" in sd:
        y = y + F.conv1d(x.double(), sd[prefix + "w2.weight"].double(), sd[prefix + "w2.bias"].double())
    return F.gelu(y)


def case_ref(name, g, sd=None, x=None, p=None, vb=None):
    """The restatement's output for fixture case `name` (tensors default to the fixture's own)."""
    sd = g["state_dict"] if sd is None else sd
    x = g["x"] if x is None else x
    p = g.get("p") if p is None else p
    vb = g.get("vb") if vb is None else vb
    if name.startswith("fno_layer1d"):
        return fno_layer1d_ref(sd, "", x, p)
    if name.startswith("fno1d"):
        h = x
        for i in range(g["kwargs"]["hidden_blocks"]):
            h_in = torch.cat([h.double(), vb.double()], dim=1) if vb is not None else h
            h = fno_layer1d_ref(sd, f"fno_layers.{i}.", h_in, p)
        return h
    return _conv(sd, "", x, p, g["kwargs"].get("transform_mode", 1))


SPECTRAL = [n + s for n in ("spectral1d_a", "spectral1d_nyq", "spectral1d_odd") for s in ("", "_tm0", "_tm1")]
CASES = SPECTRAL + ["fno_layer1d", "fno_layer1d_double", "fno1d_film", "fno1d_concat"]


def build_module(name, kwargs):
    """The product module of a fixture case, constructed as make_golden_1d.py constructs the reference's."""
    from models.enc_proc_dec_components.proc_fno import SpectralConv1d, FNO_Layer, FNO
    torch.manual_seed(42)
    if name.startswith("fno_layer1d"):
        return FNO_Layer(**kwargs)
    if name.startswith("fno1d"):
        return FNO(pde=None, **kwargs)
    return SpectralConv1d(**dict(kwargs, modes=tuple(kwargs["modes"])))


def call_module(name, m, x, p=None, vb=None):
    if name.startswith("fno1d"):
        return m(x, variables=p, variables_broadcast=vb)
    return m(x, p)
