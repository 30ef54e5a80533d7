"""Host checks of the exact-fp32 conv test tables (tests/conv_f32_cases.py): what nps_conv2d_plan picks under
NPS_PREC_F32 for every row, that the rows together reach every fp32 kernel instantiation and every stage count of the
producer/consumer ring, and that no row's reference is degenerate.  No GPU."""
import pytest
import torch

import conv_f32_cases as cf

PLANNED = [c for c in cf.FORWARD_CASES if not c.forced]
FORCED = [c for c in cf.FORWARD_CASES if c.forced]


@pytest.mark.parametrize("name", [c.name for c in PLANNED])
def test_row_plans_to_its_label(name):
    """A planner change that moves a row off the kernel it was written for fails here, not silently on the GPU."""
    c = cf.FORWARD_BY_NAME[name]
    assert c.planned() == c.plan, (c.kernel, c.planned())
    assert c.plan in cf.ALL_TILES


def test_rows_cover_every_instantiation_and_tile():
    assert sorted({c.kernel for c in cf.FORWARD_CASES}) == cf.ALL_INSTANTIATIONS
    assert {c.plan for c in cf.FORWARD_CASES} == cf.ALL_TILES
    # conv2d_fwd_kernel<1> is reached by caller-set tiles only, in both of its shapes
    assert {c.plan for c in FORCED} == {(1, 8, 8), (1, 4, 16)}
    assert all(c.plan[1] * c.plan[2] == 64 * c.plan[0] for c in FORCED)
    assert all(c.planned()[0] != 1 for c in FORCED)


def test_ring_stage_counts_are_present():
    """1, 2, 3, 4, 5 and 7 K stages for the 16-channel-stage kernels (3x3, 2x2) and the 32-channel-stage 1x1, a
    4-channel tail and a Cin % 4 != 0 source (fetch4) for each."""
    for k in (1, 2, 3):
        rows = [c for c in PLANNED if c.k == k and c.plan[0] == 8]
        assert {1, 2, 3, 4, 5, 7} <= {c.stages for c in rows}, (k, sorted({c.stages for c in rows}))
        assert any(c.Cin % 16 == 4 for c in rows), k
        assert any(len(c.srcs) == 1 and c.Cin % 4 for c in rows), k
    # the kernel's own arithmetic, spelled out for the table's channel counts
    assert [cf.FORWARD_BY_NAME[n].stages for n in ("pc3x3_8x16", "pc3x3_st2_co5", "pc3x3_st7_co6")] == [1, 2, 7]
    assert [cf.FORWARD_BY_NAME[n].stages for n in ("pc1x1", "pc1x1_st2_co75", "pc1x1_st7_co75")] == [1, 2, 7]


def test_cout_tails_are_present():
    for k, want in ((3, {5, 64, 68, 193}), (2, {5, 64, 68, 193}), (1, {75, 192, 193, 388})):
        have = {c.Cout for c in PLANNED if c.k == k and c.plan[0] == 8}
        assert want <= have, (k, want - have)
        assert any(c % 4 for c in have), k


def test_planner_never_picks_one_wave():
    """Recorded finding: over this sweep of geometries the generic kernel serves (3x3 strided or dilated, 4x4, 5x5)
    nps_conv2d_plan returns waves 2 or 4, never 1 — the 2-wave 8x16 candidate always offers at least as many waves
    as the 1-wave tiles behind it and comes first.  conv2d_fwd_kernel<1> is reachable only through a caller-set
    tile.  If this starts failing the planner changed: give the new waves == 1 shape a row in the table."""
    seen = {}
    for k in (3, 4, 5):
        for stride in (1, 2):
            for dil in (1, 2):
                if k == 3 and stride == 1 and dil == 1:
                    continue  # the producer/consumer kernel's geometry
                for Cout in (8, 64, 200):
                    for B in (1, 2, 5):
                        for H in range(6, 70, 3):
                            for W in range(6, 70):
                                if min(H, W) <= dil * (k - 1):
                                    continue
                                w, th, tw = cf.plan_f32(B, 8, Cout, k, H, W, stride=stride, dil=dil)
                                seen[(w, th, tw)] = seen.get((w, th, tw), 0) + 1
    assert set(seen) <= {(4, 16, 16), (4, 8, 32), (2, 8, 16)}, seen
    assert (2, 8, 16) in seen and (4, 16, 16) in seen


@pytest.mark.parametrize("name", [c.name for c in cf.FORWARD_CASES])
def test_forward_reference_is_not_degenerate(name):
    """fp64 reference nonzero on the written region, the fp32 CPU result differs from it (a nonzero error to scale
    the GPU's by), and the unwritten region is non-empty exactly where a row claims to leave something untouched."""
    c = cf.FORWARD_BY_NAME[name]
    ref64, cpu32 = cf.forward_refs(name)
    m = cf.touched_mask(c)
    assert m.any()
    assert torch.linalg.vector_norm(ref64[m]) > 0
    assert (ref64[m] != 0).double().mean() > 0.9        # not zeroed by GELU, cropping or padding
    e32 = cf.rel_l2_on(cpu32, ref64, m)
    assert 0 < e32 < 1e-5, e32
    assert torch.equal(ref64[~m].float(), cf.forward_inputs(name).prefill[~m])
    leaves = c.out_os != 1 or c.out_C is not None or c.out_off != (0, 0)
    assert bool((~m).any()) == leaves


@pytest.mark.parametrize("name", [c.name for c in cf.WGRAD_CASES])
def test_wgrad_reference_is_not_degenerate(name):
    ref64, cpu32 = cf.wgrad_refs(name)
    c = cf.WGRAD_BY_NAME[name]
    assert tuple(ref64.shape) == (c.M, c.N, c.k, c.k)
    assert torch.linalg.vector_norm(ref64) > 0 and (ref64 != 0).all()
    assert 0 < cf.rel_l2_on(cpu32, ref64) < 1e-5


def test_wgrad_cases_cover_the_kernel_paths():
    ks = {(c.k, c.dil) for c in cf.WGRAD_CASES}
    assert {(1, 1), (2, 1), (3, 1), (5, 1), (5, 2), (5, 4)} <= ks
    assert {20, 64, 68, 132} <= {c.M for c in cf.WGRAD_CASES} and {20, 64, 68, 132} <= {c.N for c in cf.WGRAD_CASES}
    assert any(c.M % 4 and c.N % 4 for c in cf.WGRAD_CASES)
    assert any(c.B == 1 and (c.Ha, c.Wa) == (4, 16) for c in cf.WGRAD_CASES)
    assert any(c.seeded for c in cf.WGRAD_CASES)
    assert any(c.pad and c.k == k for c in cf.WGRAD_CASES for k in (1, 2, 3))
    assert any(c.circ and c.k < 5 for c in cf.WGRAD_CASES)


def test_precision_context_restores_on_error():
    from nps_hip import ops
    old = ops.CONV_PRECISION
    with pytest.raises(ZeroDivisionError):
        with cf.f32_precision():
            assert ops.CONV_PRECISION == ops.PREC_F32
            assert ops.conv_precision(3, 3) == ops.PREC_F32
            1 / 0
    assert ops.CONV_PRECISION == old
