"""approx_volume_preserve_mode 'block' and 'individual' on the GPU (csrc/volume.hip: nps_volume_factors,
nps_volume_apply, nps_volume_factors_bwd, nps_volume_apply_bwd; reference activation_wrapper.py:40-79), stage by stage
against the fp64 restatement of tests/volume_ref.py and through the wrapper against the reference's own output
(tests/golden/volume_modes.pt).

The synthetic planes are scaled so that the tanh argument z = (1 - s / p) 100 / m cycles through saturated,
transitional and near-linear values (volume_ref.case asserts it), on ragged planes, planes with several blocks each,
tw = 1 and B * c = 65, with a two-channel mask read at channel 1.  The bound is the project's 1e-5, flat, forward and
backward: the factor kernels keep every scalar in fp64, so the cancellation 1 - s / p divided by m / 100, which costs
fp32 torch up to 2.5e-4 in the backward at m = 1/25, does not reach the result.
"""
import functools
import types

import pytest
import torch
from torch import nn

import volume_ref as V
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _dev(t):
    return None if t is None else t.to(DEV)


def _stage_forward(case):
    """plane_sums x 2, the factor kernel and the apply kernel as the wrapper's inference path calls them"""
    from nps_hip import ops
    B, c, tw, H, W = case["u"].shape
    u, x = case["u"].to(DEV), case["x"].to(DEV)
    new_tot = ops.plane_sums(u, 0, H * W, H * W, B * c * tw)
    prev_tot = ops.plane_sums(x, (V.T_IN - 1) * H * W, V.T_IN * H * W, H * W, B * c)
    F = ops.volume_factors(new_tot, prev_tot, case["mode"], case["m"], B, c, tw)
    return ops.volume_apply(u.clone(), F, _dev(case["mask"]), V.MASK_CH)


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("m", V.M_VALUES, ids=["m1", "m0.04"])
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", V.SHAPES, ids=str)
def test_stage_forward_vs_fp64(shape, mode, m, with_mask):
    """Measured on an MI355X, rel-L2 against fp64, the worst over shapes, m and mask on / off:
    block 3.0e-08 (m = 1) and 3.4e-08 (m = 1/25), individual 3.0e-08 and 3.3e-08."""
    case = V.case(shape, m, mode, with_mask)
    err = rel_l2(_stage_forward(case), case["ref"])
    print(f"volume fwd {shape} {mode} m={m:g} mask={with_mask}: rel-L2 {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("gkind", ["randn", "correlated"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("m", V.M_VALUES, ids=["m1", "m0.04"])
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("shape", V.SHAPES, ids=str)
def test_stage_backward_vs_fp64(shape, mode, m, with_mask, gkind):
    """VolumeModeFn (forward and backward) vs fp64 autograd of the restatement; the error of fp32 CPU torch autograd of
    the same formula on the same inputs is printed for the record, it is no part of the bound.  Measured on an MI355X,
    rel-L2 against fp64 of the kernels / of fp32 CPU torch, each the worst over shapes and mask on / off:
        block      m = 1:    randn 3.3e-08 / 1.0e-06, correlated 4.4e-08 / 1.4e-05
        block      m = 1/25: randn 3.4e-08 / 1.9e-05, correlated 5.4e-08 / 1.7e-04
        individual m = 1:    randn 3.2e-08 / 1.0e-06, correlated 5.3e-08 / 1.3e-05
        individual m = 1/25: randn 3.5e-08 / 4.0e-05, correlated 4.9e-08 / 2.9e-04"""
    from nps_hip import autograd as ad
    case = V.case(shape, m, mode, with_mask)
    gy = V.upstream(case["u"], gkind)
    x_last = case["x"][:, :, -1]
    _, ref = V.autograd(case["u"], x_last, gy, m, mode, case["mask"], torch.float64)
    _, g32 = V.autograd(case["u"], x_last, gy, m, mode, case["mask"], torch.float32)
    u = case["u"].to(DEV).requires_grad_(True)
    y = ad.VolumeModeFn.apply((V.MASK_CH, mode, m), u, case["x"].to(DEV), _dev(case["mask"]))
    y.backward(gy.to(DEV))
    err, err32 = rel_l2(u.grad, ref), rel_l2(g32, ref)
    print(f"volume bwd {shape} {mode} m={m:g} mask={with_mask} g={gkind}: kernel {err:.3e}, fp32 CPU torch {err32:.3e}")
    assert rel_l2(y, case["ref"]) < TOL
    assert err < TOL


@pytest.mark.parametrize("mode", V.MODES)
def test_gradient_couples_the_time_steps(mode):
    """Shape 2, m = 1, every z in the near-linear band (|z| = 0.4 or 0.45: dp_{i+1}/dp_i ~ tanh(z)^2 shrinks with z, so
    the band's upper end keeps the chain's share of the gradient visible).  'individual': an upstream gradient on the
    last step alone reaches step 0 through the chain of p_i (lambda of the reverse recurrence); 'block': one on step
    0 alone reaches every step through the mean total (the 1 / tw).  A dropped lambda leaves exact zeros at t = 0, a
    missing 1 / tw a factor tw.  Measured on an MI355X: 'individual', the gradient at t = 0 is 3.2e-03 of the whole
    norm, rel-L2 2.6e-09; 'block', the gradient at each t > 0 is 5.4e-02 of the norm, rel-L2 1.2e-09, and 2.7e-08 at
    t = 0."""
    from nps_hip import autograd as ad
    shape = V.SHAPES[1]
    tw = shape[2]
    u0, x, mask = V.make_inputs(shape, 1.0, mode, seed=515, z_targets=(-0.45, 0.4, 0.45, -0.4))
    assert (V.realised_z(u0, x[:, :, -1], 1.0, mode) < 0.5).all()
    src = tw - 1 if mode == "individual" else 0
    gy = torch.zeros_like(u0)
    gy[:, :, src] = V.upstream(u0, "correlated")[:, :, src]
    _, ref = V.autograd(u0, x[:, :, -1], gy, 1.0, mode, mask, torch.float64)
    u = u0.to(DEV).requires_grad_(True)
    ad.VolumeModeFn.apply((V.MASK_CH, mode, 1.0), u, x.to(DEV), mask.to(DEV)).backward(gy.to(DEV))
    got = u.grad.cpu()
    for t in ([0] if mode == "individual" else range(tw)):
        share = (ref[:, :, t].norm() / ref.norm()).item()
        err = rel_l2(got[:, :, t], ref[:, :, t])
        print(f"volume coupling {mode}: upstream on t={src}, gradient at t={t}: {share:.3e} of the norm, rel-L2 {err:.3e}")
        assert ref[:, :, t].abs().min() > 0 and got[:, :, t].abs().min() > 0
        assert err < TOL
    assert rel_l2(got, ref) < TOL


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
def test_one_step_window_is_one_function_in_every_mode(with_mask):
    """tw = 1 (shape 3), m = 1: 'block', 'individual' and the 'individual_static' kernels with the one-entry table [m]
    compute the same function.  Each within 1e-5 of fp64 and of one another, forward and backward.  Measured on an
    MI355X, forward / backward, the worse of mask on and off: 'block' and 'individual' 3.0e-08 / 5.0e-08 (equal to
    every printed digit), 'individual_static' 6.3e-08 / 2.5e-06."""
    from nps_hip import autograd as ad
    shape, m = V.SHAPES[2], 1.0
    case = V.case(shape, m, "individual", with_mask)
    assert rel_l2(V.forward(case["u"].double(), case["x"][:, :, -1].double(), m, "block",
                            None if case["mask"] is None else case["mask"].double()), case["ref"]) < 1e-14
    gy = V.upstream(case["u"], "correlated")
    _, gref = V.autograd(case["u"], case["x"][:, :, -1], gy, m, "individual", case["mask"], torch.float64)
    ys, gs = {}, {}
    for mode in V.MODES + ("individual_static",):
        u = case["u"].to(DEV).requires_grad_(True)
        if mode == "individual_static":
            y = ad.VolumeRescaleFn.apply(V.MASK_CH, u, case["x"].to(DEV), torch.tensor([m], device=DEV),
                                         _dev(case["mask"]))
        else:
            y = ad.VolumeModeFn.apply((V.MASK_CH, mode, m), u, case["x"].to(DEV), _dev(case["mask"]))
        y.backward(gy.to(DEV))
        ys[mode], gs[mode] = y.detach(), u.grad
        e_y, e_g = rel_l2(y, case["ref"]), rel_l2(u.grad, gref)
        print(f"volume tw=1 {mode} mask={with_mask}: forward {e_y:.3e}, backward {e_g:.3e}")
        assert e_y < TOL and e_g < TOL
    for a in ys:
        for b in ys:
            assert rel_l2(ys[a], ys[b]) < TOL and rel_l2(gs[a], gs[b]) < TOL, (a, b)


# ------------------------------------------------------------------ through the wrapper
@functools.lru_cache(maxsize=None)
def _wrapped(mode, with_mask):
    import models
    g = load_golden("volume_modes")["model"]
    m = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), activation=nn.GELU(),
                                  pde=types.SimpleNamespace(**g["pde"]), enforce_spatial_cond=with_mask,
                                  spatial_cond_channel=0, approx_volume_preserve=True,
                                  approx_volume_preserve_mode=mode, max_pct_dif=1, **g["kwargs"])
    m.load_state_dict(g["state_dict"], strict=True)
    return g, m.to(DEV)


def _call(m, g):
    return m(x=g["x"].to(DEV), cond=g["cond"].to(DEV), bc=None, pos=g["pos"].to(DEV), t_cond=None,
             spatial_cond=g["spatial_cond"].to(DEV))


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("mode", V.MODES)
def test_wrapped_model_vs_reference(mode, with_mask):
    """The wrapped EncProcDec against the reference's output (fp32, and the reference run in fp64), bound 1e-5 as for
    the wrapped-model goldens of test_gpu_parity.py; inference (in place on u) and the grad-enabled path (VolumeModeFn)
    agree within the same bound.  Measured on an MI355X, against the reference in fp64 / in fp32: 'block'
    8.7e-08 / 1.4e-07, 'individual' 1.4e-07 / 1.9e-07; the two paths of either mode agree bit for bit."""
    g, m = _wrapped(mode, with_mask)
    rec = g[f"{mode}/{'mask' if with_mask else 'nomask'}"]
    with torch.no_grad():
        y_inf = _call(m, g)
    y_ad = _call(m, g)
    assert y_ad.requires_grad and not y_inf.requires_grad and type(m).__name__ == "ActWrapper-EncProcDec"
    errs = dict(inference_vs_fp64=rel_l2(y_inf, rec["y64"]), inference_vs_fp32=rel_l2(y_inf, rec["y"]),
                grad_vs_fp64=rel_l2(y_ad, rec["y64"]), grad_vs_inference=rel_l2(y_ad, y_inf))
    print(f"wrapped {mode} mask={with_mask}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    if with_mask:
        assert (y_inf.cpu()[g["spatial_cond"][:, :1, None].expand_as(y_inf) > 0] == 0).all()


def test_default_mode_is_block():
    """approx_volume_preserve=True without a mode is 'block', as in the reference (activation_wrapper.py:13)."""
    import models
    g, m = _wrapped("block", True)
    d = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), activation=nn.GELU(),
                                  pde=types.SimpleNamespace(**g["pde"]), enforce_spatial_cond=True,
                                  spatial_cond_channel=0, approx_volume_preserve=True, **g["kwargs"])
    d.load_state_dict(g["state_dict"], strict=True)
    with torch.no_grad():
        assert torch.equal(_call(d.to(DEV), g), _call(m, g))


@pytest.mark.parametrize("mode", V.MODES)
def test_one_optimiser_step(mode):
    """One Adam step through the wrapper: a finite loss, finite gradients, every parameter moved."""
    import models
    g = load_golden("volume_modes")["model"]
    torch.manual_seed(7)
    m = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), activation=nn.GELU(),
                                  pde=types.SimpleNamespace(**g["pde"]), enforce_spatial_cond=True,
                                  spatial_cond_channel=0, approx_volume_preserve=True,
                                  approx_volume_preserve_mode=mode, max_pct_dif=1, **g["kwargs"]).to(DEV).train()
    m.load_state_dict(g["state_dict"], strict=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    target = torch.rand(g["x"].shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    loss = (_call(m, g) - target).pow(2).sum().sqrt()
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).all(), k
    opt.step()
    print(f"volume optimiser step {mode}: loss {loss.item():.4f}")
    for k, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
