"""Stage-level fp64 checks of the 'individual_static' volume preservation (activation_wrapper.py:80-105;
nps_plane_sums, nps_volume_rescale, nps_plane_dot, nps_volume_rescale_bwd) and of the encoder input packing
(nps_pack_grid_input).

The model goldens only reach these kernels with randomly initialised models, whose volume drifts by far more
than max_pct_dif per step: the tanh argument z = (1 - new_tot / prev) * 100 / mpd_t has |z| >= 27 on every
plane, where 1 - tanh(z)^2 is exactly 0 in fp32, so the df/ds term of the backward (and the slope of the forward)
contributes nothing.  Here the planes of u are scaled so that z cycles through saturated, transitional and
near-linear values, on ragged planes, planes large enough for several blocks per plane (atomic partial sums),
and with a two-channel mask read at channel 1.  Every reference is plain torch on the CPU in fp64, computed from
the same fp32 inputs.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

Z_TARGETS = (-40.0, -3.0, -1.0, -0.3, 0.0, 0.3, 1.0, 3.0, 40.0)
# (B, c, tw, H, W): a ragged 437-element plane; a 2115-element plane (plane_sums / plane_dot: 2 blocks per plane
# adding atomically, volume_rescale(_bwd): 3)
SHAPES = [(2, 3, 25, 19, 23), (1, 1, 25, 47, 45)]
T_IN = 3  # time steps of the model input x: prev_tot reads its last one through a strided view
MASK_CH = 1


def _mpd_table(kind, tw):
    """fp32 cumsum of max_pct_dif (activation_wrapper.py:87-88): 1/25 in the twophase cfgs, 1 by default."""
    step = np.float32(0.04 if kind == "twophase" else 1.0)
    return torch.from_numpy(np.cumsum(np.full(tw, step, dtype=np.float32), dtype=np.float32))


def _reference(u, x_last, mpd, mask):
    """oracle/model.py:75-88 on whatever dtype the arguments carry."""
    new_tot = u.sum((3, 4))
    prev = x_last.sum((2, 3))[:, :, None]
    dif = torch.tanh((1 - new_tot / prev) * 100 / mpd) / 100 * mpd
    v = u / new_tot[..., None, None] * ((1 - dif) * prev)[..., None, None]
    if mask is not None:
        m = mask[:, MASK_CH][:, None, None]
        v = v - m * v
    return v


@functools.lru_cache(maxsize=None)
def _case(shape, table, with_mask):
    """fp32 CPU inputs whose planes realise every z of Z_TARGETS, and the fp64 reference output."""
    B, c, tw, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + (7 if table == "twophase" else 0))
    mpd = _mpd_table(table, tw)
    x = torch.rand(B, c, T_IN, H, W, generator=g)
    prev = x[:, :, -1].double().sum((2, 3))                                       # (B, c)
    u64 = torch.rand(B, c, tw, H, W, generator=g, dtype=torch.float64)
    z = torch.tensor(Z_TARGETS, dtype=torch.float64)[torch.arange(B * c * tw) % len(Z_TARGETS)].view(B, c, tw)
    want = prev[:, :, None] * (1 - z * mpd.double() / 100)
    u = (u64 * (want / u64.sum((3, 4)))[..., None, None]).float()
    mask = None
    if with_mask:
        mask = (torch.rand(B, 2, H, W, generator=g) < 0.3).float()
        mask[:, 0] = 1 - mask[:, 1]  # channel 0 differs everywhere: a wrong channel shows
    # the realised z must populate the linear, transitional and saturated bands, or this file degenerates to
    # what the model goldens already cover
    zr = ((1 - u.double().sum((3, 4)) / prev[:, :, None]) * 100 / mpd.double()).abs()
    assert (zr < 0.5).any() and ((zr >= 0.5) & (zr <= 3)).any() and (zr > 20).any(), zr
    ref = _reference(u.double(), x[:, :, -1].double(), mpd.double(), None if mask is None else mask.double())
    return dict(u=u, x=x, mpd=mpd, mask=mask, ref=ref)


def _upstream(case, kind):
    g = torch.Generator().manual_seed(99)
    r = torch.randn(case["u"].shape, generator=g)
    # correlated with u: only then is D = sum g (1 - m) u large enough for the coef term to carry weight
    return r if kind == "randn" else case["u"] + 0.1 * r


def _autograd_ref(case, gy, dtype):
    u = case["u"].to(dtype, copy=True).requires_grad_(True)
    mask = None if case["mask"] is None else case["mask"].to(dtype)
    _reference(u, case["x"][:, :, -1].to(dtype), case["mpd"].to(dtype), mask).backward(gy.to(dtype))
    return u.grad


@pytest.mark.parametrize("shape", SHAPES)
def test_plane_sums_vs_fp64(shape):
    """nps_plane_sums accumulates in fp64 like the reference: 1e-12 per plane, for the contiguous planes of u and
    for the strided last-time-step planes of x (activation_wrapper.py:84)."""
    from nps_hip import ops
    case = _case(shape, "default", False)
    B, c, tw, H, W = shape
    u, x = case["u"].to(DEV), case["x"].to(DEV)
    new_tot = ops.plane_sums(u, 0, H * W, H * W, B * c * tw).cpu()
    prev_tot = ops.plane_sums(x, (T_IN - 1) * H * W, T_IN * H * W, H * W, B * c).cpu()
    ref_new = case["u"].double().sum((3, 4)).flatten()
    ref_prev = case["x"][:, :, -1].double().sum((2, 3)).flatten()
    e_new = ((new_tot - ref_new).abs() / ref_new.abs()).max().item()
    e_prev = ((prev_tot - ref_prev).abs() / ref_prev.abs()).max().item()
    print(f"plane_sums {shape}: max rel per plane new_tot {e_new:.2e}, prev_tot (strided) {e_prev:.2e}")
    assert e_new < 1e-12 and e_prev < 1e-12


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("table", ["twophase", "default"])
@pytest.mark.parametrize("shape", SHAPES)
def test_volume_rescale_forward_vs_fp64(shape, table, with_mask):
    """plane_sums x 2 + nps_volume_rescale as activation_wrapper.py:61-64 calls them, in every tanh regime."""
    from nps_hip import ops
    case = _case(shape, table, with_mask)
    B, c, tw, H, W = shape
    u, x = case["u"].to(DEV), case["x"].to(DEV)
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    new_tot = ops.plane_sums(u, 0, H * W, H * W, B * c * tw)
    prev_tot = ops.plane_sums(x, (T_IN - 1) * H * W, T_IN * H * W, H * W, B * c)
    y = ops.volume_rescale(u.clone(), new_tot, prev_tot, case["mpd"].to(DEV), mask, MASK_CH).cpu()
    err = rel_l2(y, case["ref"])
    print(f"volume_rescale fwd {shape} {table} mask={with_mask}: rel-L2 {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("gkind", ["randn", "correlated"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("table", ["twophase", "default"])
@pytest.mark.parametrize("shape", SHAPES)
def test_volume_rescale_backward_vs_fp64(shape, table, with_mask, gkind):
    """VolumeRescaleFn.backward (nps_plane_dot + nps_volume_rescale_bwd) vs fp64 autograd of the reference.

    Bound: the project's 1e-5 with the default table.  With the twophase table (mpd_0 = 0.04) no fp32 evaluation of
    the reference formula reaches 1e-5 for a gradient correlated with u: 1 - new_tot / prev cancels and is then divided
    by mpd, so the bound is max(1e-5, 4 x the error of fp32 CPU torch autograd of the same formula on the same inputs)
    — the factor 4 for the kernel's different rounding of that one ill-conditioned scalar (its fp64 plane sums are
    cast to fp32 where torch sums in fp32).  Measured on an MI355X, rel-L2 against fp64 of the kernel / of fp32 CPU
    torch, each the worst over both shapes and mask on / off:
        default table:  randn 6.4e-08 / 9.5e-08, correlated 4.3e-07 / 1.6e-06
        twophase table: randn 4.5e-07 / 4.9e-07, correlated 1.7e-05 / 1.3e-05
    (the twophase correlated case with the largest kernel error: 1.68e-05 against 1.13e-05, bound 4.5e-05)."""
    from nps_hip import autograd as ad
    case = _case(shape, table, with_mask)
    gy = _upstream(case, gkind)
    ref = _autograd_ref(case, gy, torch.float64)
    u = case["u"].to(DEV).requires_grad_(True)
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    y = ad.VolumeRescaleFn.apply(MASK_CH, u, case["x"].to(DEV), case["mpd"].to(DEV), mask)
    y.backward(gy.to(DEV))
    err = rel_l2(u.grad, ref)
    err32 = rel_l2(_autograd_ref(case, gy, torch.float32), ref)
    bound = 1e-5 if table == "default" else max(1e-5, 4 * err32)
    print(f"volume_rescale bwd {shape} {table} mask={with_mask} g={gkind}: kernel {err:.3e}, fp32 CPU torch "
          f"{err32:.3e}, bound {bound:.3e}")
    assert rel_l2(y, case["ref"]) < 1e-5
    assert err < bound


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", SHAPES)
def test_plane_dot_vs_fp64(shape, with_mask):
    """D[plane] = sum g (1 - m) u.  The kernel rounds each product to fp32 (relative 2^-24; the 0/1 mask is exact)
    and adds in fp64, so |D - D_ref| <= 2^-24 sum |g (1 - m) u| up to the fp64 accumulation (0.1 % headroom)."""
    from nps_hip import lib, ptr, stream_ptr, check
    case = _case(shape, "default", with_mask)
    B, c, tw, H, W = shape
    for gkind in ("randn", "correlated"):
        gy = _upstream(case, gkind)
        t = gy.double() * case["u"].double()
        if with_mask:
            t = t * (1 - case["mask"][:, MASK_CH].double())[:, None, None]
        ref, slack = t.sum((3, 4)).flatten(), 1.001 * 2.0 ** -24 * t.abs().sum((3, 4)).flatten()
        gd, ud = gy.to(DEV), case["u"].to(DEV)
        md = case["mask"].to(DEV) if with_mask else None
        D = torch.full((B * c * tw,), float("nan"), dtype=torch.float64, device=DEV)
        check(lib.nps_plane_dot(ptr(gd), ptr(ud), ptr(md), 2 if with_mask else 0, MASK_CH, B, c * tw, H, W, ptr(D),
                                stream_ptr()), "plane_dot")
        over = ((D.cpu() - ref).abs() / slack).max().item()
        print(f"plane_dot {shape} mask={with_mask} g={gkind}: max |D - ref| / (2^-24 sum|terms|) = {over:.3f}")
        assert over <= 1.0


# ------------------------------------------------------------------ encoder input packing
@pytest.mark.parametrize("B,c,tw,H,W,K,S,Cp", [
    (2, 3, 25, 9, 7, 2, 1, 84),     # HW = 63: one ragged 64-pixel block
    (1, 1, 25, 13, 10, 0, 2, 32),   # K = 0, S = 2, 130 pixels: a 2-pixel tail block
    (2, 2, 4, 8, 8, 3, 0, 16),      # S = 0
    (1, 2, 3, 5, 6, 0, 0, 8),       # K = S = 0: vb untouched
])
def test_pack_grid_input_exact(B, c, tw, H, W, K, S, Cp):
    """xin = [u flattened | pos | cond broadcast | spatial cond | zeros] in NHWC and vb = [cond | spatial cond]
    (enc_proc_dec.py:127-137, enc_grid.py:41-47): copies only, so exact."""
    from nps_hip import ops, lib, ptr, stream_ptr, check
    g = torch.Generator().manual_seed(B * 100 + H)
    u = torch.randn(B, c, tw, H, W, generator=g)
    pos = torch.rand(B, H, W, 2, generator=g)
    cond = torch.randn(B, K, generator=g) if K else None
    sc = torch.randn(B, S, H, W, generator=g) if S else None
    parts = [u.flatten(1, 2), pos.movedim(-1, 1)]
    vparts = []
    if K:
        vparts.append(cond[:, :, None, None].expand(B, K, H, W))
    if S:
        vparts.append(sc)
    n = c * tw + 2 + K + S
    xin_ref = torch.cat(parts + vparts + [torch.zeros(B, Cp - n, H, W)], dim=1).permute(0, 2, 3, 1)
    ud, posd = u.to(DEV), pos.to(DEV)
    if K + S:
        xin, vb = ops.pack_grid_input(ud, posd, None if cond is None else cond.to(DEV),
                                      None if sc is None else sc.to(DEV), Cp)
        assert torch.equal(vb.cpu(), torch.cat(vparts, dim=1).permute(0, 2, 3, 1))
    else:  # the C entry point with a vb buffer it must not touch
        xin = torch.full((B, H, W, Cp), float("nan"), device=DEV)
        vb = torch.full((B, H, W, 1), float("nan"), device=DEV)
        check(lib.nps_pack_grid_input(ptr(ud), ptr(posd), None, None, ptr(xin), ptr(vb), B, c * tw, H, W, 0, 0, Cp,
                                      stream_ptr()), "pack_grid_input")
        assert torch.isnan(vb).all()
    assert torch.equal(xin.cpu(), xin_ref)
