"""The grid decoders on the MI355X (csrc/decode_chain.hip: nps_decode_fwd / nps_decode_bwd; dec_grid.TimeConvLinear,
TimeConv, TimeConvDense with dec_delta_mode 'all' / 'none', LinearConv, add_delta) against fp64: the restatement
tests/decoders_ref.py (pinned to the reference's recorded results by test_decoders_host.py) and the reference's own
EncProcDec outputs and gradients (tests/golden/decoders_epd_*.pt).

Tolerance: rel-L2 < 1e-5 per tensor, forward and every gradient, the bar of test_gpu_timeconv_bwd.py.  Every chain
here is a few dozen fp32 FMAs per output and the reference's own fp32 error on the fixtures' shapes is 3e-8 .. 6e-6
(e_ref in the fixtures), so no tensor gets an allowance.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import load_golden, rel_l2
import decoders_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def _check(errs, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (what, bad)


# ------------------------------------------------------------------ the chain kernel, directly
# (nstage, C0, L0, C1, k1, s1, act, beta, C2, k2) -> num_c x tw, then (delta_mode, dt, tanh, mask)
CHAINS = {
    "two_gelu_per_step_tanh_mask": (dict(C0=2, L0=15, C1=4, k1=3, s1=2, act=1, C2=2, k2=3), "per_step", 0.3, True, True),
    "two_swish_all": (dict(C0=1, L0=32, C1=8, k1=5, s1=2, act=2, beta=0.7, C2=3, k2=10), "all", 0.3, False, False),
    "one_none_tanh": (dict(C0=3, L0=12, C1=3, k1=3, s1=2), "none", 0.3, True, False),
    "one_stride3_all_mask": (dict(C0=2, L0=16, C1=2, k1=4, s1=3), "all", 0.3, False, True),
    "zero_per_step_nodt_mask": (dict(C0=2, L0=5), "per_step", 1, False, True),   # dec_delta_dt=False: dt = 1
    "zero_all_tanh_mask": (dict(C0=3, L0=4), "all", 0.3, True, True),
    "zero_none": (dict(C0=1, L0=7), "none", 0.3, False, False),
}


def _chain_sizes(c):
    if "C1" not in c:
        return c["C0"], c["L0"]
    L1 = (c["L0"] - c["k1"]) // c["s1"] + 1
    return (c["C2"], L1 - c["k2"] + 1) if "C2" in c else (c["C1"], L1)


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "channels_last"])
@pytest.mark.parametrize("N", [1, 67, 130])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_kernel_vs_fp64(name, N, planar):
    """N = 1 (one pixel), 67 (one full group of 64 and a ragged one), 130 (more than two); B = 2."""
    from nps_hip import ops
    from nps_hip import autograd as ad
    from models.enc_proc_dec_components.dec_grid import dt_cumsum
    c, mode, dt, tanh, use_mask = CHAINS[name]
    B, C0, L0 = 2, c["C0"], c["L0"]
    num_c, tw = _chain_sizes(c)
    g = torch.Generator().manual_seed(1000 * list(CHAINS).index(name) + N)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    x = rnd(B, C0 * L0, N) if planar else rnd(B, N, C0 * L0)
    u = torch.rand(B, num_c, tw, N, generator=g)
    mask = (torch.rand(B, 2, N, generator=g) > 0.6).float() if use_mask else None
    if use_mask:
        mask[0, :, 0] = 0  # (one pixel stays unmasked at N = 1: the output and the gradients are not all zero)
    w1 = rnd(c["C1"], C0, c["k1"]) * 0.5 if "C1" in c else None
    b1 = rnd(c["C1"]) * 0.5 if "C1" in c else None
    w2 = rnd(c["C2"], c["C1"], c["k2"]) * 0.5 if "C2" in c else None
    b2 = rnd(c["C2"]) * 0.5 if "C2" in c else None
    gy = rnd(B, num_c, tw, N)
    act = {0: None, 1: F.gelu, 2: lambda z: R.swish(z, c.get("beta", 1.0))}[c.get("act", 0)]
    params = [t for t in (w1, b1, w2, b2) if t is not None]

    def ref(x64, *ps):
        ps = list(ps) + [None] * (4 - len(ps))
        px = (torch.movedim(x64, 1, -1) if planar else x64).reshape(B * N, C0, L0)
        d = R.chain(px, ps[0], ps[1], c.get("s1", 1), act, ps[2], ps[3])
        d = d.reshape(B, N, num_c, tw).permute(0, 2, 3, 1)
        return R.wrap(R.add_delta(d, u.double(), dt, mode), tanh, mask[:, 1].double() if use_mask else None)
    y64, grads64 = R.reference(ref, [x] + params, gy)

    spec = ops.DecodeSpec(planar=planar, C0=C0, L0=L0, num_c=num_c, tw=tw, delta_mode=ops.DELTA_MODES[mode],
                          dt=float(dt), s1=c.get("s1", 1), act=c.get("act", 0), beta=c.get("beta", 1.0),
                          act_tanh=tanh, mask_ch=1)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    dtcum = torch.from_numpy(dt_cumsum(dt, tw)).to(DEV) if mode == "per_step" else None
    xd = x.to(DEV).requires_grad_(True)
    pd = [dev(t).requires_grad_(True) if t is not None else None for t in (w1, b1, w2, b2)]
    y = ad.DecodeChainFn.apply(spec, xd, u.to(DEV), *pd, dtcum, dev(mask))
    y_inf = ops.decode_chain(spec, x.to(DEV), u.to(DEV), dev(w1), dev(b1), dev(w2), dev(b2), dtcum, dev(mask))
    assert torch.equal(y.detach(), y_inf)
    y.backward(gy.to(DEV))
    errs = dict(y=rel_l2(y, y64), x=rel_l2(xd.grad, grads64[0]))
    for nm, p, gr in zip(("w1", "b1", "w2", "b2"), [q for q in pd if q is not None], grads64[1:]):
        errs[nm] = rel_l2(p.grad, gr)
    _check(errs, f"chain {name} N={N} {'planar' if planar else 'channels-last'}")


def test_chain_backward_is_bit_reproducible_and_skips_null_gradients():
    """Two runs give identical bits (no atomics); gradients that are not asked for are not computed (x only)."""
    from nps_hip import ops
    from nps_hip import autograd as ad
    g = torch.Generator().manual_seed(3)
    B, N = 2, 1000
    x = torch.randn(B, N, 32, generator=g).to(DEV)
    u = torch.rand(B, 3, 5, N, generator=g).to(DEV)
    w1, b1 = torch.randn(8, 1, 5, generator=g).to(DEV), torch.randn(8, generator=g).to(DEV)
    w2, b2 = torch.randn(3, 8, 10, generator=g).to(DEV) * 0.2, torch.randn(3, generator=g).to(DEV)
    gy = torch.randn(B, 3, 5, N, generator=g).to(DEV)
    spec = ops.DecodeSpec(planar=False, C0=1, L0=32, num_c=3, tw=5, delta_mode=1, dt=0.3, s1=2, act=2)
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
        ad.DecodeChainFn.apply(spec, leaves[0], u, *leaves[1:], None, None).backward(gy)
        runs.append([t.grad for t in leaves])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    xd = x.clone().requires_grad_(True)
    ad.DecodeChainFn.apply(spec, xd, u, w1, b1, w2, b2, None, None).backward(gy)
    assert torch.equal(xd.grad, runs[0][0])


# ------------------------------------------------------------------ the modules against the restatement
def _decoder(cls, kw, dt=0.3, beta=None, seed=11):
    from models.enc_proc_dec_components import dec_grid
    extra = {} if cls in ("TimeConv", "LinearConv") else dict(activation=nn.GELU())
    torch.manual_seed(seed)
    m = getattr(dec_grid, cls)(pde=types.SimpleNamespace(dt=dt), **kw, **extra)
    if beta is not None:
        m.decoder[1].beta = beta
    return m


def _module_vs_fp64(cls, kw, spatial, dt=0.3, beta=None, what=""):
    """forward without grad, forward + backward in grad mode: y, the gradient of h and of every parameter."""
    m = _decoder(cls, kw, dt, beta)
    g = torch.Generator().manual_seed(12)
    h = torch.randn(2, kw["hidden_features"], *spatial, generator=g)
    u = torch.rand(2, kw["num_c"], kw["time_window"], *spatial, generator=g)
    gy = torch.randn(2, kw["num_c"], kw["time_window"], *spatial, generator=g)
    rkw = dict(kw, **({} if beta is None else dict(beta=beta)))
    y64, gh64, grads64 = R.reference_sd(lambda sd, h64: R.decoder(cls, sd, h64, u.double(), dt, rkw), m.state_dict(), h,
                                        gy)
    m = m.to(DEV)
    with torch.no_grad():
        y_inf = m(h.to(DEV), u.to(DEV))
    hd = h.to(DEV).requires_grad_(True)
    y = m(hd, u.to(DEV))
    assert y.shape == u.shape and y.requires_grad and not y_inf.requires_grad
    y.backward(gy.to(DEV))
    errs = dict(y_inference=rel_l2(y_inf, y64), y=rel_l2(y, y64), h=rel_l2(hd.grad, gh64))
    for k, p in m.named_parameters():
        errs[k] = rel_l2(p.grad, grads64[k])
    _check(errs, what or f"{cls} {kw} {spatial}")


@pytest.mark.parametrize("num_c", [1, 3])
@pytest.mark.parametrize("tw", [1, 4, 5, 8])
def test_timeconvlinear(tw, num_c):
    """tw = 1: the special case of decoder_input_dim; tw = 4, 8: an even kernel; 7 x 9 pixels."""
    mode = {1: "all", 4: "none", 5: "per_step", 8: "per_step"}[tw]
    _module_vs_fp64("TimeConvLinear", dict(num_c=num_c, num_spatial_dims=2, time_window=tw, hidden_features=16,
                                           dec_delta_mode=mode), (7, 9))


@pytest.mark.parametrize("num_c", [1, 2])
@pytest.mark.parametrize("hidden,tw,N", [(16, 5, 130), (32, 5, 130), (48, 4, 67), (128, 25, 67)])
def test_timeconv(hidden, tw, N, num_c):
    """(stride, kernel) = (1, 3), (2, 5), (3, 10), (3, 27): the last are the cfgs' sizes (hidden 128, tw 25)."""
    _module_vs_fp64("TimeConv", dict(num_c=num_c, num_spatial_dims=1, time_window=tw, hidden_features=hidden), (N,),
                    dt=0.1 if tw == 25 else 0.3)


def test_timeconv_swish_beta():
    _module_vs_fp64("TimeConv", dict(num_c=2, num_spatial_dims=1, time_window=5, hidden_features=32,
                                     dec_delta_mode="all"), (67,), beta=0.5)


@pytest.mark.parametrize("mode", ["all", "none"])
@pytest.mark.parametrize("num_c,tw", [(2, 8), (3, 25)])
def test_timeconvdense_all_none(num_c, tw, mode):
    _module_vs_fp64("TimeConvDense", dict(num_c=num_c, num_spatial_dims=1, time_window=tw, hidden_features=16,
                                          dec_delta_mode=mode), (67,), dt=0.1 if tw == 25 else 0.3)


def test_timeconvdense_per_step_keeps_its_kernel():
    """per_step + GELU is still nps_timeconv_decode: bit-equal to ops.timeconv_decode on the module's own
    pre-decoder output."""
    from nps_hip import ops
    from models.common import run_pointwise
    m = _decoder("TimeConvDense", dict(num_c=3, num_spatial_dims=2, time_window=25, hidden_features=16), dt=0.1).to(DEV)
    g = torch.Generator().manual_seed(13)
    h = torch.randn(2, 7, 9, 16, generator=g).to(DEV)
    u = torch.rand(2, 3, 25, 7, 9, generator=g).to(DEV)
    with torch.no_grad():
        y = m.run(h, u)
        pre = run_pointwise(m.pre_decoder, [ops.Src(h)], out_nchw=True)
        c1, c2 = m.decoder[0], m.decoder[2]
        want = ops.timeconv_decode(pre, u, c1.weight.contiguous(), c1.bias, c2.weight.contiguous(), c2.bias,
                                   m._dtcum(h.device), None, 0, False, 3, 25)
    assert torch.equal(y, want)


@pytest.mark.parametrize("pad", ["zeros", "circular"])
@pytest.mark.parametrize("k", [1, 3])
def test_linearconv_2d(k, pad):
    _module_vs_fp64("LinearConv", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=16,
                                       dec_kernel_size=k, dec_padding_mode=pad), (7, 9))


def test_linearconv_1d():
    _module_vs_fp64("LinearConv", dict(num_c=2, num_spatial_dims=1, time_window=5, hidden_features=16,
                                       dec_kernel_size=3, dec_padding_mode="zeros", dec_delta_mode="all"), (13,))


GRIDS = {"1d": (37,), "2d": (7, 9), "3d": (3, 4, 5)}
FORWARDS = [(cls, grid) for cls in ("TimeConvLinear", "TimeConv", "TimeConvDense", "LinearConv") for grid in GRIDS
            if not (cls == "LinearConv" and grid == "3d")]


@pytest.mark.parametrize("cls,grid", FORWARDS)
def test_forward_on_every_grid(cls, grid):
    """forward in both grad modes on a 1-D (L = 37), a 2-D (7 x 9) and a 3-D (3 x 4 x 5) grid."""
    spatial = GRIDS[grid]
    kw = dict(num_c=2, num_spatial_dims=len(spatial), time_window=5, hidden_features=32 if cls == "TimeConv" else 16)
    if cls == "LinearConv":
        kw.update(dec_kernel_size=3, dec_padding_mode="zeros" if grid == "1d" else "circular")
    if cls == "TimeConvDense":
        kw.update(dec_delta_mode="all")
    _module_vs_fp64(cls, kw, spatial)


@pytest.mark.parametrize("mode,delta_dt", [("per_step", True), ("per_step", False), ("all", True), ("none", True)])
def test_add_delta_function(mode, delta_dt):
    from models.enc_proc_dec_components.dec_grid import add_delta
    g = torch.Generator().manual_seed(14)
    delta = torch.randn(2, 3, 5, 7, 9, generator=g)
    u = torch.rand(2, 3, 5, 7, 9, generator=g)
    gy = torch.randn(2, 3, 5, 7, 9, generator=g)
    y64, (gd64,) = R.reference(lambda d: R.add_delta(d, u.double(), 0.3, mode, delta_dt), [delta], gy)
    with torch.no_grad():
        y_inf = add_delta(delta.to(DEV), u.to(DEV), 0.3, 5, 2, delta_mode=mode, delta_dt=delta_dt)
    dd = delta.to(DEV).requires_grad_(True)
    y = add_delta(dd, u.to(DEV), 0.3, 5, 2, delta_mode=mode, delta_dt=delta_dt)
    y.backward(gy.to(DEV))
    _check(dict(y_inference=rel_l2(y_inf, y64), y=rel_l2(y, y64), delta=rel_l2(dd.grad, gd64)), f"add_delta {mode}")


# ------------------------------------------------------------------ EncProcDec against the reference's fixtures
EPD = ["tcl", "tc", "tcd_none", "lc", "tcl_wrapped"]


@functools.lru_cache(maxsize=None)
def _epd(name):
    import models
    g = load_golden(f"decoders_epd_{name}")
    grads = load_golden(f"decoders_epd_{name}_grads")
    pde = types.SimpleNamespace(**g["pde"])
    if g["wrapper"] is None:
        m = models.EncProcDec(pde=pde, activation=nn.GELU(), **g["kwargs"])
    else:
        m = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), pde=pde,
                                      activation=nn.GELU(), **g["wrapper"], **g["kwargs"])
    m.load_state_dict(g["state_dict"], strict=True)
    return g, grads, m.to(DEV)


def _call(m, g):
    return m(x=g["x"].to(DEV), cond=g["cond"].to(DEV), bc=None, pos=g["pos"].to(DEV), t_cond=None,
             spatial_cond=g["spatial_cond"].to(DEV))


@pytest.mark.parametrize("name", EPD)
def test_encprocdec_inference(name):
    g, _, m = _epd(name)
    with torch.no_grad():
        y = _call(m, g)
    _check(dict(y=rel_l2(y, g["y64"])), f"EncProcDec {name} inference")
    if g["wrapper"] is not None:
        assert type(m).__name__ == "ActWrapper-EncProcDec"
        assert (y.cpu()[g["spatial_cond"][:, :1, None].expand_as(y.cpu()) > 0] == 0).all() and y.abs().max() <= 1


@pytest.mark.parametrize("name", EPD)
def test_encprocdec_trains(name):
    g, grads, m = _epd(name)
    for p in m.parameters():
        p.grad = None
    y = _call(m, g)
    assert y.requires_grad
    y.backward(g["g"].to(DEV))
    got = dict(m.named_parameters())
    assert set(got) == set(grads)
    errs = dict(y=rel_l2(y, g["y64"]), **{k: rel_l2(got[k].grad, v) for k, v in grads.items()})
    _check(errs, f"EncProcDec {name} grad mode")


# ------------------------------------------------------------------ one pushforward training step per decoder
@pytest.mark.parametrize("decoder,extra", [
    ("TimeConvLinear", {}), ("TimeConv", dict(hidden_features=32)), ("TimeConvDense", dict(dec_delta_mode="all")),
    ("LinearConv", dict(dec_kernel_size=3, dec_padding_mode="circular"))])
def test_pushforward_training_step(decoder, extra):
    """AutoregressivePushforwardTrainer.train_one_epoch on one batch (the trainer of test_gpu_trainer.py) with Adam:
    a finite loss and every parameter moved."""
    import argparse
    import random
    import models
    from common.interfaces import D
    from pdes import PDE2D
    from trainers.autoregressivepushforwardtrainer import AutoregressivePushforwardTrainer
    from trainers.synthetic import twophase_batch
    random.seed(0)
    torch.manual_seed(5)
    tw, res = 5, 16
    pde = PDE2D(tmin=0.0, tmax=1.0, nt=11, L1=1.0, L2=1.0, nx1=res, nx2=res, x=None, name="twophase",
                n_cond_static=3, n_cond_spatial=1)
    kw = dict(model_class="EncProcDec", activation_final=nn.Tanh(), enforce_spatial_cond=True, spatial_cond_channel=0,
              num_c=2, num_spatial_dims=2, time_window=tw, encoder="enc_grid.ElementWise", activation=nn.GELU(),
              processor="FNO", fno_modes=2, hidden_blocks=1, hidden_features=16, fno_kernel_size=1,
              fno_conv_mode="single", decoder=f"dec_grid.{decoder}")
    kw.update(extra)
    m = models.activation_wrapper(**kw, pde=pde).to(DEV).train()
    u, cond, pos, sc = twophase_batch(2, 2, 2 * tw, res, res, seed=3, obstacle="random", device=DEV)
    batch = (u[:, :, :1], u, pos, cond, torch.empty(u.shape[0], 0, device=DEV), sc)
    cfg = argparse.Namespace(time_window=tw, base_resolution=(2 * tw, res, res), device=DEV, batch_size=2,
                             lr_step_interval=1, unrolling=2)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    tr = AutoregressivePushforwardTrainer(model=m, data=types.SimpleNamespace(pde=pde, data_interface=D.sim2d),
                                          criterion=nn.MSELoss(reduction="sum"), optimizer=opt, config=cfg)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss = float(tr.train_one_epoch([batch], epoch=0))
    assert loss == loss and 0 < loss < 1e6, loss
    for k, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[k]), f"{k} not updated"


# ------------------------------------------------------------------ what is still refused
def test_remaining_refusals_come_before_any_launch():
    """Models on the GPU, inputs on the CPU: a launch (or its device check) would raise a RuntimeError instead."""
    m = _decoder("LinearConv", dict(num_c=1, num_spatial_dims=3, time_window=2, hidden_features=4, dec_kernel_size=3,
                                    dec_padding_mode="zeros")).to(DEV)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="LinearConv.*3-D"):
            m(torch.zeros(1, 4, 3, 4, 5), torch.zeros(1, 1, 2, 3, 4, 5))
    from models.enc_proc_dec_components.dec_grid import TimeConvDense
    m = TimeConvDense(pde=types.SimpleNamespace(dt=0.1), num_c=2, num_spatial_dims=2, time_window=5,
                      hidden_features=16, activation=nn.ReLU(), dec_delta_mode="all").to(DEV)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="GELU"):
            m(torch.zeros(1, 16, 4, 4), torch.zeros(1, 2, 5, 4, 4))
