"""The exact-fp32 conv path (NPS_CONV_PRECISION=f32) on the GPU: every fp32 forward kernel instantiation and
nps_conv2d_wgrad against fp64, the launch audit, existing module / model parity tests collected again under the f32
switch, and the host paths only that mode takes.  The whole module runs with ops.CONV_PRECISION = PREC_F32 (autouse
fixture below); tables, references and drivers are in tests/conv_f32_cases.py, the host side of the tables in
tests/test_conv_f32_host.py.

Bounds.  (1) rel-L2 against the fp64 CPU reference < 1e-5, the project's parity bar.  (2) "Exact fp32" is the mode's
claim, so the error must also be of fp32's own class: rel_l2(gpu, ref64) <= F_CLASS * rel_l2(cpu32, ref64), cpu32 the
same operation by torch in fp32 on the CPU.  F_CLASS = 8: measured on an MI355X over all rows (profiles/conv_f32/
ratios.jsonl) the ratio lies in [0.69, 2.53] for the forward rows (rel-L2 4.6e-8 .. 4.2e-7) and in [0.45, 1.22] for the
weight gradients (rel-L2 1.3e-7 .. 3.6e-7); the smallest power of two >= 2 x the largest ratio is 8.  The ratio grows
with the length of the K loop (2.5 at Cin = 100, 3x3: 900 products added one after the other into one MFMA
accumulator, where the CPU's blocked GEMM adds partial sums), as sequential fp32 summation does."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_f32_cases as cf
from conftest import rel_l2
from oracle import functional as Fo

# existing parity tests, collected a second time here so they run under the f32 fixture (their assertions unchanged)
from test_gpu_parity import test_conv2d_vs_torch as test_f32_conv2d_vs_torch  # noqa: F401
from test_gpu_parity import test_conv_transpose_vs_torch as test_f32_conv_transpose_vs_torch  # noqa: F401
from test_gpu_parity import (  # noqa: F401
    test_residual_block_concat_crop_groupnorm as test_f32_residual_block_concat_crop_groupnorm)
from test_gpu_parity import test_conv1x1_planar_output_vs_torch as test_f32_conv1x1_planar_output_vs_torch  # noqa: F401
from test_gpu_parity import test_processor_golden as test_f32_processor_golden  # noqa: F401
from test_gpu_backward import test_conv2d_backward_vs_torch as test_f32_conv2d_backward_vs_torch  # noqa: F401
from test_gpu_backward import (  # noqa: F401
    test_conv_transpose_backward_vs_torch as test_f32_conv_transpose_backward_vs_torch)
from test_gpu_backward import (  # noqa: F401
    test_residual_block_backward_concat_crop_groupnorm as test_f32_residual_block_backward_concat_crop_groupnorm)
from test_gpu_backward import test_processor_backward_vs_oracle as test_f32_processor_backward_vs_oracle  # noqa: F401
from test_gpu_backward import test_conv1x1_channel_groups_vs_fp64 as test_f32_conv1x1_channel_groups_vs_fp64  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = cf.DEV
TOL = cf.TOL
F_CLASS = 8.0


@pytest.fixture(autouse=True)
def _f32_mode():
    with cf.f32_precision():
        yield


def test_the_fixture_selects_fp32():
    from nps_hip import ops
    assert ops.CONV_PRECISION == ops.PREC_F32
    assert ops.conv_precision(3, 3) == ops.conv_precision(1, 1) == ops.conv_precision(5, 5, 1, 2) == ops.PREC_F32


# ------------------------------------------------------------------ a + b: forward rows and their launch audit
@pytest.mark.parametrize("name", [c.name for c in cf.FORWARD_CASES])
def test_forward_row_vs_fp64(name):
    """One table row through ops.pack_conv_weight + ops.conv2d (conv2d_fwd_kernel<1> rows: a hand-filled nps_conv2d_t)
    against the fp64 CPU reference; the recorded launch is the exact-fp32 kernel with the waves the host test pinned
    (not split-fp16 behind a stale packing); everything of `out` the launch must not touch keeps its bits."""
    c = cf.FORWARD_BY_NAME[name]
    ref64, cpu32 = cf.forward_refs(name)
    got, launches = cf.run_forward(c)
    assert launches == [("f32", c.k * c.k, c.plan[0])], (c.kernel, launches)
    m = cf.touched_mask(c)
    assert torch.equal(got[~m], cf.forward_inputs(name).prefill[~m])
    err, e32 = cf.rel_l2_on(got, ref64, m), cf.rel_l2_on(cpu32, ref64, m)
    print(f"conv_f32 forward {name} {c.kernel} rel_l2 {err:.3e} cpu32 {e32:.3e} ratio {err / e32:.3f}")
    assert err < TOL, (err, e32)
    assert err <= F_CLASS * e32, (err, e32, err / e32)


# ------------------------------------------------------------------ c: weight gradient
@pytest.mark.parametrize("name", [c.name for c in cf.WGRAD_CASES])
def test_wgrad_f32_vs_fp64(name):
    """ad.wgrad -> nps_conv2d_wgrad (wgrad_kernel, exact fp32 MFMA, split-K atomics) against
    torch.nn.grad.conv2d_weight in fp64 on the extended frame; a given g is added to."""
    c = cf.WGRAD_BY_NAME[name]
    ref64, cpu32 = cf.wgrad_refs(name)
    got, launches = cf.run_wgrad(c)
    assert launches == [("f32w", c.k * c.k, 0)], launches
    err, e32 = cf.rel_l2_on(got, ref64), cf.rel_l2_on(cpu32, ref64)
    print(f"conv_f32 wgrad {name} rel_l2 {err:.3e} cpu32 {e32:.3e} ratio {err / e32:.3f}")
    assert err < TOL, (err, e32)
    assert err <= F_CLASS * e32, (err, e32, err / e32)


# ------------------------------------------------------------------ e: host paths only f32 takes
def _nchw64(t):
    return t.detach().cpu().double()


def _conv3x3():
    from models.common import Conv2d
    return Conv2d(20, 24, 3, padding=1), torch.randn(2, 20, 17, 19), \
        lambda m, x: F.conv2d(x, _nchw64(m.weight), _nchw64(m.bias), padding=1)


def _downsample():
    from models.common import Conv2d
    return Conv2d(32, 40, 3, stride=2, padding=1), torch.randn(2, 32, 21, 18), \
        lambda m, x: F.conv2d(x, _nchw64(m.weight), _nchw64(m.bias), stride=2, padding=1)


def _conv_transpose():
    from models.common import ConvTranspose2d
    return ConvTranspose2d(24, 20, kernel_size=4, stride=2, padding=1), torch.randn(2, 24, 13, 11), \
        lambda m, x: F.conv_transpose2d(x, _nchw64(m.weight), _nchw64(m.bias), stride=2, padding=1)


@pytest.mark.parametrize("make", [_conv3x3, _downsample, _conv_transpose], ids=["conv3x3", "s2d_downsample", "convT"])
def test_in_place_weight_update_repacks_the_fp32_packing(make, monkeypatch):
    """cached_pack with a stale exact-fp32 packing (no batched repack job: _nps_job is None): after an in-place
    weight update the next forward uses the new weights.  The Downsample runs over the materialised space_to_depth
    copy, the transposed conv as four launches — both f32-only host paths."""
    from nps_hip import ops
    torch.manual_seed(11)
    m, x, ref = make()
    m = m.to(DEV)
    xd = x.to(DEV)
    copies, real_s2d = [], ops.space_to_depth
    monkeypatch.setattr(ops, "space_to_depth", lambda *a, **k: copies.append(1) or real_s2d(*a, **k))
    ops.conv_probe = []
    try:
        y0 = m(xd).cpu()
        n_launch = len(ops.conv_probe)
        assert all(p[3][0] == "f32" for p in ops.conv_probe)
    finally:
        ops.conv_probe = None
    assert n_launch == (4 if make is _conv_transpose else 1)
    assert len(copies) == (1 if make is _downsample else 0)
    assert rel_l2(y0, ref(m, x.double())) < TOL
    packs = [v[1] for v in m.weight._nps_packs.values()]
    assert packs and all(getattr(t, "_nps_job", 0) is None
                         for p in packs for t in (p if isinstance(p, list) else [p]))
    with torch.no_grad():
        m.weight.mul_(1.5)
    y1 = m(xd).cpu()
    assert rel_l2(y1, ref(m, x.double())) < TOL
    assert rel_l2(y1, y0) > 0.1          # (the update is visible: the stale packing would reproduce y0)


def test_precision_round_trip_on_one_module():
    """x3f16 -> f32 -> x3f16 on one Conv2d and the same input: each result within the bar of fp64, the two split-fp16
    results bit-identical (the f32 packing in between leaked into neither), the f32 result different bits."""
    from models.common import Conv2d
    from nps_hip import ops
    torch.manual_seed(12)
    m = Conv2d(36, 40, 3, padding=1).to(DEV)
    x = torch.randn(2, 36, 20, 22)
    ref = F.conv2d(x.double(), _nchw64(m.weight), _nchw64(m.bias), padding=1)
    xd = x.to(DEV)
    ys = []
    for prec in (ops.PREC_X3F16, ops.PREC_F32, ops.PREC_X3F16):
        old = ops.CONV_PRECISION
        ops.CONV_PRECISION = prec
        ops.conv_probe = []
        try:
            ys.append(m(xd).cpu())
            assert [p[3][0] for p in ops.conv_probe] == ["x3f16" if prec == ops.PREC_X3F16 else "f32"]
        finally:
            ops.conv_probe = None
            ops.CONV_PRECISION = old
    assert all(rel_l2(y, ref) < TOL for y in ys), [rel_l2(y, ref) for y in ys]
    assert torch.equal(ys[0], ys[2])
    assert not torch.equal(ys[0], ys[1])


def test_residual_block_groupnorm_moments_fall_back_to_the_stats_pass(monkeypatch):
    """ResidualBlock(norm=True) under f32: no fp32 kernel carries GroupNorm moments, so every out_stats buffer handed
    to a conv is marked incomplete, no output carries moments and norm2's statistics come from nps_group_norm_stats;
    forward and backward match the oracle."""
    from models.enc_proc_dec_components.proc_unet_modern import ResidualBlock
    from nps_hip import autograd as ad
    from nps_hip import ops
    torch.manual_seed(13)
    rb = ResidualBlock(20, 24, activation=nn.GELU(), norm=True, num_spatial_dims=2,
                       padding_kwargs=dict(padding_mode="circular"))
    with torch.no_grad():
        for n in (rb.norm1, rb.norm2):
            n.weight.uniform_(0.5, 1.5)
            n.bias.uniform_(-0.3, 0.3)
    h = torch.randn(2, 20, 18, 21)
    sd = {k: t.detach().clone().requires_grad_(True) for k, t in rb.state_dict().items()}
    hr = h.clone().requires_grad_(True)
    ref = Fo.residual_block(sd, "", hr, True, dict(padding_mode="circular"))
    g = torch.randn_like(ref)
    ref.backward(g)
    rb = rb.to(DEV)

    handed, passes = [], []
    real_conv, real_stats = ops.conv2d, ops.lib.nps_group_norm_stats
    monkeypatch.setattr(ops, "conv2d", lambda *a, **k: handed.append(k.get("out_stats")) or real_conv(*a, **k))
    monkeypatch.setattr(ops.lib, "nps_group_norm_stats", lambda *a: passes.append(1) or real_stats(*a))
    hd = ops.nchw_to_nhwc(h.to(DEV))
    y = rb.run([ops.Src(hd)], (18, 21))
    handed = [st for st in handed if st is not None]
    assert len(handed) >= 2 and all(getattr(st, "_nps_incomplete", False) for st in handed)
    assert ops.stats_of(y) is None
    assert len(passes) >= 2              # norm1 over the input, norm2 over conv1's output
    assert rel_l2(ops.nhwc_to_nchw(y), ref) < TOL
    assert ad._carry_buffer(hd) is None

    hg = hd.clone().requires_grad_(True)
    ya = rb.run_ad([ops.Src(hg)], (18, 21))
    ya.backward(ops.nchw_to_nhwc(g.to(DEV)))
    assert rel_l2(ops.nhwc_to_nchw(ya.detach()), ref) < TOL
    assert rel_l2(ops.nhwc_to_nchw(hg.grad), hr.grad) < TOL
    got = dict((k, p.grad) for k, p in rb.named_parameters())
    allg = torch.cat([got[k].cpu().double().flatten() for k in sd])
    allr = torch.cat([sd[k].grad.double().flatten() for k in sd])
    assert rel_l2(allg, allr) < TOL


def test_spectral_fusion_is_off_under_f32():
    from nps_hip import ops
    assert not ops.spectral_fusable(256, 10, 192)
