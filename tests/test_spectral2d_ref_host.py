"""The fp64 restatement of the SpectralConv2d stages (tests/spectral2d_ref.py) is itself checked, on the CPU: its
stages composed with a plain einsum mixer against the module formula irfft2(P(rfft2(x))) of proc_fno.py:257-288 in
complex128 under torch autograd (output, dx, dweights1, dweights2), and its 3-D weight packing against the four
corner writes of proc_fno.py:342-350.  Both sides are fp64, so they agree to rounding: the bar is rel-L2 < 1e-12.
"""
import pytest
import torch

from conftest import rel_l2
import spectral2d_ref as R

TOL = 1e-12


def _module2d(x, w1, w2):
    """SpectralConv2d.forward on channels-first x (B, Cin, H, W), complex128."""
    m1, m2 = w1.shape[-2], w1.shape[-1]
    x_ft = torch.fft.rfft2(x)
    out_ft = torch.zeros(x.shape[0], w1.shape[1], x.size(-2), x.size(-1) // 2 + 1, dtype=torch.complex128)
    out_ft[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, :m1, :m2], w1)
    out_ft[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, -m1:, :m2], w2)
    return torch.fft.irfft2(out_ft, s=(x.size(-2), x.size(-1)))


def _cplx(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g, dtype=torch.float64),
                         torch.randn(*shape, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("B,H,W,Cin,Cout,m1,m2", [
    (2, 6, 8, 3, 4, 4, 5),      # overlapping corners (R = H), even W with the Nyquist bin retained
    (1, 8, 7, 3, 2, 3, 4),      # odd W with m2 = W // 2 + 1
    (1, 40, 12, 2, 2, 17, 3),   # R = 34 > 32 retained rows
])
def test_stages_compose_to_the_module_formula(B, H, W, Cin, Cout, m1, m2):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    w1, w2 = _cplx(g, Cin, Cout, m1, m2), _cplx(g, Cin, Cout, m1, m2)
    gy = torch.randn(B, H, W, Cout, generator=g, dtype=torch.float64)

    def grads(fn, xin, to_nhwc):
        leaves = [xin.clone().requires_grad_(), w1.clone().requires_grad_(), w2.clone().requires_grad_()]
        y = to_nhwc(fn(*leaves))
        return (y.detach(),) + torch.autograd.grad(y, leaves, gy)

    got = grads(R.spectral2d, x, lambda y: y)
    want = grads(_module2d, x.permute(0, 3, 1, 2).contiguous(), lambda y: y.permute(0, 2, 3, 1))
    want = (want[0], want[1].permute(0, 2, 3, 1)) + want[2:]
    for name, a, b in zip(("y", "dx", "dw1", "dw2"), got, want):
        err = rel_l2(a, b)
        print(f"spectral2d_ref vs irfft2(P(rfft2)) H={H} W={W} m1={m1} m2={m2} {name}: rel-L2 {err:.3e}")
        assert err < TOL, name
    if 2 * m1 > H:  # weights1 rows that the [-m1:] corner overwrites never reach the output
        assert (got[2][:, :, H - m1:] == 0).all() and (got[2][:, :, :H - m1] != 0).all()


@pytest.mark.parametrize("D,H,m1,m2", [
    (8, 9, 2, 3),   # no overlap
    (3, 9, 2, 3),   # corners overlap along D only
    (8, 4, 2, 3),   # along H only
    (3, 5, 2, 3),   # along both
    (2, 3, 2, 3),   # D == m1 and H == m2: the last write owns every mode
])
def test_pack3d_is_the_four_corner_writes(D, H, m1, m2):
    """P(X) of proc_fno.py:342-350 on a random spectrum X against the retained modes of X mixed with pack3d's
    weights and scattered back, and the four weight gradients of both under a random cotangent."""
    B, Cin, Cout, m3 = 2, 2, 3, 2
    g = torch.Generator().manual_seed(D * 10 + H)
    X = _cplx(g, B, Cin, D, H, m3)
    G = _cplx(g, B, Cout, D, H, m3)
    ws = [_cplx(g, Cin, Cout, m1, m2, m3) for _ in range(4)]
    mul = lambda a, w: torch.einsum("bixyz,ioxyz->boxyz", a, w)

    def module(w1, w2, w3, w4):
        out = torch.zeros(B, Cout, D, H, m3, dtype=torch.complex128)
        out[:, :, :m1, :m2] = mul(X[:, :, :m1, :m2], w1)
        out[:, :, -m1:, :m2] = mul(X[:, :, -m1:, :m2], w2)
        out[:, :, :m1, -m2:] = mul(X[:, :, :m1, -m2:], w3)
        out[:, :, -m1:, -m2:] = mul(X[:, :, -m1:, -m2:], w4)
        return out

    def restated(w1, w2, w3, w4):
        r1, r2 = R.k1_rows(D, m1), R.k1_rows(H, m2)
        wp = R.pack3d(w1, w2, w3, w4, D, H)                       # (R1, R2, m3, Cin, Cout)
        Y = torch.einsum("bipqz,pqzio->bopqz", X[:, :, r1][:, :, :, r2], wp)
        rows = torch.zeros(B, Cout, len(r1), H, m3, dtype=torch.complex128).index_add(3, torch.tensor(r2), Y)
        return torch.zeros(B, Cout, D, H, m3, dtype=torch.complex128).index_add(2, torch.tensor(r1), rows)

    def run(fn):
        leaves = [w.clone().requires_grad_() for w in ws]
        out = fn(*leaves)
        return (out.detach(),) + torch.autograd.grad(out, leaves, G)

    for name, a, b in zip(("P(X)", "dw1", "dw2", "dw3", "dw4"), run(restated), run(module)):
        if name == "dw4" or b.abs().max() > 0:
            err = rel_l2(a, b)
            print(f"pack3d D={D} H={H} m1={m1} m2={m2} {name}: rel-L2 {err:.3e}")
            assert err < TOL, name
        assert torch.equal(a == 0, b == 0), name   # the same modes are owned by a later corner
