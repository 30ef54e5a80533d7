"""The small kernels of csrc/backward.hip against fp64 references: channel sums (every bias gradient), circular
pad and its adjoint, GELU and its derivative.  All through the C ABI, so each launch's dispatch (quad / scalar by
channel count and pointer alignment, grid-stride wrap) is chosen by the arguments given here.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ nps_channel_sums
ROWS = [1, 255, 256, 257, 5000]  # below / at / above one 256-row block, and 20 blocks


# (C, floats off 16-B alignment): quad kernel; scalar kernel (300, 1028: its C > blockDim branch); C = 192 at a
# 4-byte offset, which must fall to the scalar kernel
@pytest.mark.parametrize("C,skew", [(4, 0), (40, 0), (192, 0), (388, 0), (1024, 0),
                                    (1, 0), (7, 0), (81, 0), (300, 0), (1028, 0), (192, 1)])
def test_channel_sums_vs_fp64(C, skew):
    """out[c] += sum over rows of x[row][c].  Inputs rand + 0.5 (no cancellation): rel 1e-5 per channel against the
    fp64 sum, on top of known non-zero contents of `out`."""
    from nps_hip import lib, ptr, stream_ptr, check
    g = torch.Generator().manual_seed(C)
    for rows in ROWS:
        x = torch.rand((rows, C), generator=g) + 0.5
        big = torch.zeros(rows * C + 4, device=DEV)
        xd = big[skew:skew + rows * C]
        xd.copy_(x.reshape(-1))
        assert xd.data_ptr() % 16 == 4 * skew
        seed = 1.0 + 0.25 * torch.arange(C, dtype=torch.float32)
        out = seed.to(DEV)
        check(lib.nps_channel_sums(xd.data_ptr(), rows, C, ptr(out), stream_ptr()), "channel_sums")
        want = seed.double() + x.double().sum(0)
        err = ((out.cpu().double() - want).abs() / want).max().item()
        print(f"channel_sums C={C} rows={rows}: {err:.3e}")
        assert err < 1e-5, (C, rows, err)


# ------------------------------------------------------------------ nps_circular_pad / nps_circular_fold
CIRC = [(C, pad) for C in (3, 8) for pad in (0, 1, 2, 5)]  # pad 5 = H: the largest the entry accepts here
CB, CH, CW = 2, 5, 7


def _pad_index(pad):
    ys = (torch.arange(CH + 2 * pad) - pad) % CH
    xs = (torch.arange(CW + 2 * pad) - pad) % CW
    return ys, xs


def _circ_pad(x, pad):
    from nps_hip import lib, ptr, stream_ptr
    out = torch.full((x.shape[0], CH + 2 * pad, CW + 2 * pad, x.shape[3]), float("nan"), device=DEV)
    return lib.nps_circular_pad(ptr(x), ptr(out), x.shape[0], CH, CW, x.shape[3], pad, stream_ptr()), out


@pytest.mark.parametrize("C,pad", CIRC)
def test_circular_pad_bit_equal_to_index_arithmetic(C, pad):
    g = torch.Generator().manual_seed(10 * C + pad)
    x = torch.randn((CB, CH, CW, C), generator=g)
    rc, out = _circ_pad(x.to(DEV), pad)
    assert rc == 0
    ys, xs = _pad_index(pad)
    assert torch.equal(out.cpu(), x[:, ys][:, :, xs])


def test_circular_pad_refuses_pad_above_size():
    from nps_hip import lib
    x = torch.zeros((CB, CH, CW, 3), device=DEV)
    rc, out = _circ_pad(x, CH + 1)
    assert rc < 0 and "circular_pad" in lib.nps_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # no launch


@pytest.mark.parametrize("C,pad", CIRC)
def test_circular_fold_is_the_adjoint_of_pad(C, pad):
    """nps_circular_fold against fp64 autograd of the index gather (rtol 1e-6: gradients rand + 0.5, so the up to
    9-term wrap sums do not cancel and fp32 keeps 8 x 2^-24 < 1e-6), and <pad(x), g> = <x, fold(g)> in fp64."""
    from nps_hip import lib, ptr, stream_ptr, check
    gen = torch.Generator().manual_seed(100 + 10 * C + pad)
    x = torch.rand((CB, CH, CW, C), generator=gen) + 0.5
    gp = torch.rand((CB, CH + 2 * pad, CW + 2 * pad, C), generator=gen) + 0.5
    ys, xs = _pad_index(pad)
    xr = x.double().requires_grad_(True)
    (xr[:, ys][:, :, xs] * gp.double()).sum().backward()
    gx = torch.full((CB, CH, CW, C), float("nan"), device=DEV)
    check(lib.nps_circular_fold(ptr(gp.to(DEV)), ptr(gx), CB, CH, CW, C, pad, stream_ptr()), "circular_fold")
    torch.testing.assert_close(gx.cpu().double(), xr.grad, rtol=1e-6, atol=0)
    rc, px = _circ_pad(x.to(DEV), pad)
    assert rc == 0
    lhs = (px.cpu().double() * gp.double()).sum().item()
    rhs = (x.double() * gx.cpu().double()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)


# ------------------------------------------------------------------ nps_gelu / nps_gelu_bwd
SPECIAL = [0.0, 1e-30, -1e-30, 3e38, -3e38]
GELU_N = [1, 2049, 4096 * 2048 + 3]  # one element; two blocks; one element past the grid cap (grid-stride wrap)


def _gelu_points(n):
    """(x, mask of the points of the dense grid over [-12, 12]): the grid plus 0, +-1e-30, +-3e38."""
    if n == 1:
        return torch.tensor([0.7]), torch.tensor([True])
    grid = torch.linspace(-12.0, 12.0, n - len(SPECIAL), dtype=torch.float64).float()
    x = torch.cat([grid, torch.tensor(SPECIAL)])
    dense = torch.ones(n, dtype=torch.bool)
    dense[-2:] = False  # (+-3e38: finite, outside the measured range)
    return x, dense


def _cpu_fp32_bar(x, gy):
    """max |error| against fp64 of fp32 CPU F.gelu and of its autograd on x (the reference class)."""
    x64 = x.double().requires_grad_(True)
    y64 = F.gelu(x64)
    y64.backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = F.gelu(x32)
    y32.backward(gy)
    return y64.detach(), x64.grad, (y32.detach().double() - y64.detach()).abs(), (x32.grad.double() - x64.grad).abs()


@pytest.mark.parametrize("n", GELU_N)
def test_gelu_forward_and_backward_vs_fp64(n):
    """nps_gelu / nps_gelu_bwd: max |error| against fp64 over the dense grid on [-12, 12] at most 4 x that of fp32 CPU
    F.gelu (and its autograd) on the same points — the two erff implementations differ by a few ulp.  Measured on
    an MI355X over the 8.4 M-point grid: forward 4.5e-7 against the CPU's 1.3e-6, derivative 2.4e-7 against 3.9e-7.
    The single-element call is held to the bar of the 2049-point grid.  Outputs at +-3e38 and +-1e-30 are finite."""
    from nps_hip import lib, ptr, stream_ptr, check
    x, dense = _gelu_points(n)
    gen = torch.Generator().manual_seed(n)
    gy = torch.rand(n, generator=gen) + 0.5
    y64, g64, ey_cpu, eg_cpu = _cpu_fp32_bar(x, gy)
    if n == 1:
        xb, db = _gelu_points(2049)
        _, _, eyb, egb = _cpu_fp32_bar(xb, torch.rand(2049, generator=gen) + 0.5)
        bar_y, bar_g = eyb[db].max().item(), egb[db].max().item()
    else:
        bar_y, bar_g = ey_cpu[dense].max().item(), eg_cpu[dense].max().item()
    xd, gyd = x.to(DEV), gy.to(DEV)
    y = torch.full((n,), float("nan"), device=DEV)
    gx = torch.full((n,), float("nan"), device=DEV)
    check(lib.nps_gelu(ptr(xd), ptr(y), n, stream_ptr()), "gelu")
    check(lib.nps_gelu_bwd(ptr(xd), ptr(gyd), ptr(gx), n, stream_ptr()), "gelu_bwd")
    y, gx = y.cpu(), gx.cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
    ey = (y.double() - y64).abs()[dense].max().item()
    eg = (gx.double() - g64).abs()[dense].max().item()
    print(f"gelu n={n}: kernel {ey:.3e} / {eg:.3e}, fp32 CPU {bar_y:.3e} / {bar_g:.3e} (forward / derivative)")
    assert ey <= 4 * bar_y, f"gelu: max |error| {ey:.3e} against fp64, fp32 CPU F.gelu {bar_y:.3e}"
    assert eg <= 4 * bar_g, f"gelu_bwd: max |error| {eg:.3e} against fp64, fp32 CPU autograd {bar_g:.3e}"
    if n > 1:  # +-3e38: gelu(x) = x or 0 and gelu'(x) = 1 or 0, to fp32 rounding
        big = torch.tensor([3e38, -3e38]).double()
        assert torch.allclose(y[-2:].double(), torch.clamp(big, min=0), rtol=1e-6, atol=0)
        assert torch.allclose(gx[-2:].double(), gy[-2:].double() * (big > 0), rtol=1e-6, atol=0)
