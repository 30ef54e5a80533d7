"""The 1-D U-Net and U-FNO on the GPU (padding_mode "ones"), module level and inside EncProcDec, against the
reference's own modules run in float64 (tests/golden/unet1d_*.pt, written by tests/golden/make_golden_unet1d.py).

Criteria.  Outputs: rel-L2 < 1e-5 of the fp64 output in both forms (inference and autograd), and the two forms agree
to 1e-6.  Parameter gradients: rel-L2 < max(1e-5, 4 * e_ref[k]) of the fp64 gradient, e_ref[k] being the rel-L2 of the
reference's own fp32 gradient against its fp64 one, recorded in the fixture (medians 0.3e-6 .. 2.6e-6, worst 8.8e-6,
a GroupNorm weight of the U-FNO model at L = 72): the HIP path is a second, independently rounded fp32 computation
with other summation orders, so it may err about as much as the reference's fp32 run and in the other direction.
Parameters the reference leaves without a gradient (the attention block's unused norm) get none here either.

Measured on an MI355X: outputs 1.0e-7 .. 7.5e-7 in both forms, the two forms within 2.6e-7 of each other; the worst
gradient error / bound per case: 0.21 (unet_l13), 0.19 (unet_l64), 0.04 (unet_plain), 0.05 (unet_nonorm), 0.30
(ufno_l37), 0.87 (epd_unet_l37), 0.49 (epd_ufno_l72).  The U-Net's pointwise convs run on the exact-fp32 Conv1d
kernels (models.common.Conv1d.exact): on the 2-D split-fp16 route 16 of epd_ufno_l72's 264 gradients lay outside the
bound (up to 1.7e-5 against 1.45e-5)."""
import functools
import types

import pytest
import torch
from torch import nn

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
CASES = ["unet_l13", "unet_l64", "unet_plain", "unet_nonorm", "ufno_l37", "epd_unet_l37", "epd_ufno_l72"]


def _build(g):
    import models
    from models.enc_proc_dec_components import UFNO, UNetModern
    if g["kind"] == "EncProcDec":
        m = models.EncProcDec(pde=types.SimpleNamespace(**g["pde"]), activation=nn.GELU(), **g["kwargs"])
    else:
        m = (UNetModern if g["kind"] == "UNetModern" else UFNO)(pde=None, activation=nn.GELU(), **g["kwargs"])
    m.load_state_dict(g["state_dict"])
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The fixture, its fp64 gradients and the model on the GPU, built once and shared (read-only)."""
    g = load_golden(f"unet1d_{name}")
    return g, load_golden(f"unet1d_{name}_grads"), _build(g)


def _call(m, g):
    dev = lambda k: g[k].to(DEV) if g.get(k) is not None else None  # noqa: E731
    if g["kind"] == "EncProcDec":
        return m(dev("x"), cond=dev("cond"), bc=None, pos=dev("pos"), t_cond=None, spatial_cond=None)
    return m(dev("x"), variables_broadcast=dev("vb"))


@pytest.mark.parametrize("name", CASES)
def test_inference_forward(name):
    g, _, m = _case(name)
    with torch.no_grad():
        y = _call(m, g)
    err = rel_l2(y, g["y64"])
    print(f"{name} inference: y rel-L2 {err:.2e} (reference fp32 {g['e_ref']['y']:.2e})")
    assert y.shape == g["y64"].shape and not y.requires_grad and err < TOL


@pytest.mark.parametrize("name", CASES)
def test_autograd_forward_and_parameter_gradients(name):
    g, grads, m = _case(name)
    for p in m.parameters():
        p.grad = None
    with torch.no_grad():
        y_inf = _call(m, g)
    y = _call(m, g)
    err, both = rel_l2(y, g["y64"]), rel_l2(y, y_inf)
    print(f"{name} grad mode: y rel-L2 {err:.2e}, against the inference form {both:.2e}")
    assert y.requires_grad and err < TOL and both < 1e-6
    y.backward(g["g"].to(DEV))
    bad, worst = [], 0.0
    for k, p in m.named_parameters():
        if k not in grads:
            assert p.grad is None, f"{k}: the reference gives it no gradient"
            continue
        assert p.grad is not None, f"no gradient for {k}"
        e, bound = rel_l2(p.grad, grads[k]), max(TOL, 4 * g["e_ref"][k])
        worst = max(worst, e / bound)
        if not e < bound:
            bad.append((k, e, bound))
    print(f"{name}: {len(grads)} parameter gradients, worst error / bound {worst:.3f}, outside: {bad}")
    assert not bad, bad


# ------------------------------------------------------------------ blocks of the first U-Net
def _maps(ts):
    """(B, C, L) -> (B, 1, L, C) on the GPU"""
    return [t.transpose(1, 2).contiguous().unsqueeze(1).to(DEV) for t in ts]


def _run_block(m, name, xs, train):
    from models.enc_proc_dec_components.proc_unet_modern import Downsample, ResidualBlock, Upsample
    from nps_hip import ops
    sub = m.get_submodule(name)
    if isinstance(sub, ResidualBlock):
        fn = sub.run_ad if train else sub.run
        return (fn([ops.Src(xs[0])], xs[0].shape[1:3]),)
    if isinstance(sub, Downsample):
        return (sub.run_ad if train else sub.run)(*xs)
    assert isinstance(sub, Upsample)
    return ((sub.conv.run_ad if train else sub.conv.run)(xs[0]),)


@pytest.mark.parametrize("train", [False, True], ids=["run", "run_ad"])
@pytest.mark.parametrize("block", ["down.0.res", "middle.res2", "down.1", "up.2"])
def test_blocks(block, train):
    """ResidualBlock with the 1x1 shortcut (down.0.res: 18 -> 16) and with the identity (middle.res2), the Downsample
    with its conditioning conv (down.1: 13 -> 7) and the Upsample (up.2: 7 -> 14), through .run / .run_ad on
    (B, 1, L, C) maps, against the reference submodule in fp64 on the same inputs"""
    g, _, m = _case("unet_l13")
    rec = g["blocks"][block]
    with torch.set_grad_enabled(train):
        outs = _run_block(m, block, _maps(rec["inputs"]), train)
    assert len(outs) == len(rec["out64"])
    for y, ref in zip(outs, rec["out64"]):
        err = rel_l2(y.squeeze(1).transpose(1, 2), ref)
        print(f"{block} {'run_ad' if train else 'run'}: rel-L2 {err:.2e}")
        assert err < TOL


# ------------------------------------------------------------------ training step, refusal
def test_one_adam_step_on_the_1d_ufno_model():
    """forward in grad mode, sqrt(MSE_sum) against a shifted target, backward, Adam: a finite loss, and every trainable
    parameter moves"""
    from nps_hip import autograd as ad
    g = load_golden("unet1d_epd_ufno_l72")
    m = _build(g).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    x = g["x"].to(DEV)
    pred = m(x, cond=g["cond"].to(DEV), bc=None, pos=g["pos"].to(DEV), t_cond=None, spatial_cond=None)
    loss = ad.sqrt_mse_sum(pred, (x.flip(3) * 0.5).contiguous())
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        assert not torch.equal(p.detach(), before[k]), k


@pytest.mark.parametrize("kind", ["UNetModern", "UFNO"])
def test_circular_1d_unet_is_refused_and_says_why(kind):
    """a one-level circular 1-D U-Net can be built (no Upsample), but has no HIP path: refused before any launch (the
    inputs are on the CPU: a launch would raise a RuntimeError about the device instead), in both grad modes, naming
    the zero-padded route and the reference's limit"""
    from models.enc_proc_dec_components import UFNO, UNetModern
    kw = dict(num_spatial_dims=1, n_cond=0, hidden_features=16, ch_mults=[1], n_blocks=1, padding_mode="circular")
    m = (UNetModern(pde=None, **kw) if kind == "UNetModern" else UFNO(pde=None, hidden_blocks=1, fno_modes=3, **kw)).to(DEV)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="'ones'.*ConvTranspose1d"):
            m(torch.zeros(1, 16, 32))


@pytest.mark.parametrize("processor", ["UNetModern", "UFNO"])
def test_encprocdec_refuses_the_circular_1d_unet_and_says_why(processor):
    """the same through EncProcDec._check_processors: the message names the processor, the dimension and the reason,
    before any launch (CPU inputs), in both grad modes"""
    import models
    kw = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", num_spatial_dims=1, num_c=1,
              time_window=5, processor=processor, hidden_features=16, cond_mode="concat", ch_mults=[1], n_blocks=1,
              padding_mode="circular", hidden_blocks=1, fno_modes=3)
    m = models.EncProcDec(pde=types.SimpleNamespace(dt=0.1, n_cond_static=0, n_cond_spatial=0), activation=nn.GELU(),
                          **kw).to(DEV)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(
                NotImplementedError, match=processor + ".*1-D.*'ones'.*ConvTranspose1d"):
            m(torch.rand(1, 1, 5, 32), pos=torch.rand(1, 32, 1))
