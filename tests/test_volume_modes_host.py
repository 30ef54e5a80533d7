"""No GPU: the restatement of approx_volume_preserve_mode 'block' / 'individual' (tests/volume_ref.py) against the
reference's own fp32 output (tests/golden/volume_modes.pt), the closed forms of the factor kernels against fp64 autograd
of that restatement, the host-side argument checks of the four nps_volume_* entries (they come before any launch), and
the wrapper's refusal of an unknown mode string."""
import ctypes
import math
import types

import pytest
import torch
from torch import nn

import volume_ref as V
from conftest import load_golden, rel_l2


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("m", V.M_VALUES, ids=["m1", "m0.04"])
@pytest.mark.parametrize("mode", V.MODES)
def test_restatement_is_the_reference(mode, m, with_mask):
    """fp64 restatement vs the reference's fp32 output on the same inputs.  Bound 1e-6: fp32 against fp64 evaluation of
    this forward differs by <= 9e-8 (measured: 6.1e-8 ... 7.6e-8 on these records), so a factor of ten is left.  The
    fp32 restatement, the same arithmetic in the same order, is within 1e-6 too."""
    g = load_golden("volume_modes")["stage"][f"{mode}/{m:g}/{'mask' if with_mask else 'nomask'}"]
    u, x_last, mask = g["u"], g["x"][:, :, -1], g["mask"] if with_mask else None
    zr = V.realised_z(u, x_last, m, mode)
    assert (zr < 0.5).any() and ((zr >= 0.5) & (zr <= 3)).any() and (zr > 20).any()
    if with_mask:  # the record's u arrives masked, as the wrapper's first mask application leaves it
        assert (u[mask[:, V.MASK_CH][:, None, None].expand_as(u) > 0] == 0).all()
    e64 = rel_l2(V.forward(u.double(), x_last.double(), m, mode, None if mask is None else mask.double()), g["y"])
    e32 = rel_l2(V.forward(u, x_last, m, mode, mask), g["y"])
    print(f"restatement {mode} m={m:g} mask={with_mask}: fp64 {e64:.3e}, fp32 {e32:.3e}")
    assert e64 < 1e-6 and e32 < 1e-6


@pytest.mark.parametrize("gkind", ["randn", "correlated"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("m", V.M_VALUES, ids=["m1", "m0.04"])
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", V.SHAPES, ids=str)
def test_closed_forms_are_autograd_of_the_restatement(shape, mode, m, with_mask, gkind):
    """out = u F and gu = g1 F + c, with F and c from the closed forms the factor kernels evaluate, against the
    restatement and its torch.autograd gradient, all in fp64: rel-L2 < 1e-10."""
    case = V.case(shape, m, mode, with_mask)
    u, x_last = case["u"].double(), case["x"][:, :, -1].double()
    mask = None if case["mask"] is None else case["mask"].double()
    gy = V.upstream(case["u"], gkind).double()
    y_ref, gu_ref = V.autograd(case["u"], case["x"][:, :, -1], gy, m, mode, case["mask"], torch.float64)
    y = u * V.factors(u.sum((3, 4)), x_last.sum((2, 3)), m, mode)[..., None, None]
    if mask is not None:
        y = y - mask[:, V.MASK_CH][:, None, None] * y
    e_y, e_g = rel_l2(y, y_ref), rel_l2(V.backward_closed_form(u, x_last, gy, m, mode, mask), gu_ref)
    print(f"closed forms {shape} {mode} m={m:g} mask={with_mask} g={gkind}: forward {e_y:.3e}, backward {e_g:.3e}")
    assert e_y < 1e-10 and e_g < 1e-10


def test_individual_with_one_step_is_the_static_formula():
    """tw = 1: lambda never leaves 0, and c is the coefficient of the 'individual_static' backward kernel,
    D ((1 - th^2) / s - f / s^2) with f = r p; 'block' is the same function there."""
    case = V.case(V.SHAPES[2], 1.0, "individual", False)
    s, p = case["u"].double().sum((3, 4)), case["x"][:, :, -1].double().sum((2, 3))
    D = torch.linspace(-1, 1, s.numel(), dtype=torch.float64).view_as(s)
    th = torch.tanh((1 - s / p[:, :, None]) * 100)
    f = (1 - th / 100) * p[:, :, None]
    want = D * ((1 - th * th) / s - f / (s * s))
    for mode in V.MODES:
        assert rel_l2(V.coefs(s, p, D, 1.0, mode), want) < 1e-12
        assert rel_l2(V.factors(s, p, 1.0, mode), f / s) < 1e-12


# ------------------------------------------------------------------ C ABI
def _call(entry, **kw):
    """One of the four entries with plausible arguments (fake non-null pointers: the checks come before any launch,
    and a call that passed them would fail at the launch, not touch the pointers on the host)."""
    import nps_hip
    a = dict(new_tot=0x1000, prev_tot=0x2000, D=0x3000, mode=0, m=1.0, ws=0x4000, F=0x5000, c=0x6000, u=0x7000,
             g=0x8000, gu=0x9000, mask=None, mask_S=0, mask_ch=0, B=2, num_c=3, tw=5, H=4, W=6)
    a.update(kw)
    lib = nps_hip.lib
    if entry == "volume_factors":
        rc = lib.nps_volume_factors(a["new_tot"], a["prev_tot"], a["mode"], a["m"], a["F"], a["B"], a["num_c"], a["tw"],
                                    None)
    elif entry == "volume_factors_bwd":
        rc = lib.nps_volume_factors_bwd(a["new_tot"], a["prev_tot"], a["D"], a["mode"], a["m"], a["ws"], a["c"],
                                        a["B"], a["num_c"], a["tw"], None)
    elif entry == "volume_apply":
        rc = lib.nps_volume_apply(a["u"], a["F"], a["mask"], a["mask_S"], a["mask_ch"], a["B"], a["num_c"], a["tw"],
                                  a["H"], a["W"], None)
    else:
        rc = lib.nps_volume_apply_bwd(a["g"], a["F"], a["c"], a["mask"], a["mask_S"], a["mask_ch"], a["gu"], a["B"],
                                      a["num_c"], a["tw"], a["H"], a["W"], None)
    return rc, lib.nps_last_error().decode()


POINTERS = {"volume_factors": ["new_tot", "prev_tot", "F"], "volume_factors_bwd": ["new_tot", "prev_tot", "D", "c"],
            "volume_apply": ["u", "F"], "volume_apply_bwd": ["g", "F", "c", "gu"]}
EXTENTS = {"volume_factors": ["B", "num_c", "tw"], "volume_factors_bwd": ["B", "num_c", "tw"],
           "volume_apply": ["B", "num_c", "tw", "H", "W"], "volume_apply_bwd": ["B", "num_c", "tw", "H", "W"]}


@pytest.mark.parametrize("entry", list(POINTERS))
def test_entries_refuse_null_pointers_and_bad_extents(entry):
    for name in POINTERS[entry]:
        rc, msg = _call(entry, **{name: None})
        assert rc < 0 and entry + ":" in msg and "null pointer" in msg, (name, msg)
    for name in EXTENTS[entry]:
        for bad in (0, -3):
            rc, msg = _call(entry, **{name: bad})
            assert rc < 0 and entry + ":" in msg and "extent" in msg, (name, bad, msg)
    rc, msg = _call(entry, B=16, num_c=64, tw=64)  # 65536 planes: one past the y extent of a launch
    assert rc < 0 and "planes" in msg


@pytest.mark.parametrize("entry", ["volume_factors", "volume_factors_bwd"])
def test_factor_entries_refuse_unknown_mode_and_bad_max_pct_dif(entry):
    for bad in (-1, 2, 7):
        rc, msg = _call(entry, mode=bad)
        assert rc < 0 and f"unknown mode {bad}" in msg, msg
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):
        for mode in (0, 1):
            rc, msg = _call(entry, mode=mode, m=bad)
            assert rc < 0 and "max_pct_dif" in msg, (bad, msg)


def test_individual_backward_needs_its_workspace():
    rc, msg = _call("volume_factors_bwd", mode=1, ws=None)
    assert rc < 0 and "null pointer" in msg and "ws" in msg


@pytest.mark.parametrize("entry", ["volume_apply", "volume_apply_bwd"])
def test_apply_entries_refuse_a_mask_channel_outside_the_mask(entry):
    for S, ch in ((2, 2), (2, -1), (0, 0)):
        rc, msg = _call(entry, mask=0xa000, mask_S=S, mask_ch=ch)
        assert rc < 0 and "mask_ch" in msg, msg


def test_max_pct_dif_is_a_double_in_the_binding():
    import nps_hip
    assert nps_hip.lib.nps_volume_factors.argtypes[3] is ctypes.c_double
    assert nps_hip.lib.nps_volume_factors_bwd.argtypes[4] is ctypes.c_double


def test_ops_refuse_cpu_tensors():
    from nps_hip import ops
    from nps_hip import autograd as ad
    u, x = torch.rand(1, 1, 2, 3, 4), torch.rand(1, 1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.volume_factors(torch.ones(2, dtype=torch.float64), torch.ones(1, dtype=torch.float64), "block", 1.0, 1, 1, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.volume_apply(u, torch.ones(1, 1, 2), None, 0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ad.VolumeModeFn.apply((0, "individual", 1.0), u.requires_grad_(True), x, None)


# ------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
def test_wrapper_refuses_an_unknown_mode_at_the_call(grad):
    """the reference's ValueError (activation_wrapper.py:103), raised before anything is launched: CPU inputs never
    reach an op"""
    import models
    pde = types.SimpleNamespace(dt=0.3, n_cond_static=1, n_cond_spatial=1)
    m = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), pde=pde, activation=nn.GELU(),
                                  approx_volume_preserve=True, approx_volume_preserve_mode="blocks",
                                  encoder="enc_grid.ElementWise", processor="FNO", num_spatial_dims=2, hidden_blocks=1,
                                  fno_modes=2, fno_kernel_size=1, fno_conv_mode="single",
                                  decoder="dec_grid.TimeConvLinear", num_c=2, time_window=5, hidden_features=8)
    x = torch.rand(2, 2, 5, 8, 8)
    pos = torch.rand(2, 8, 8, 2)
    with torch.set_grad_enabled(grad):
        with pytest.raises(ValueError, match="Unrecognized approx_volume_preserve_mode 'blocks'"):
            m(x=x, cond=torch.rand(2, 1), bc=None, pos=pos, t_cond=None, spatial_cond=torch.zeros(2, 1, 8, 8))
