"""GPU parity of the split-fp16 weight gradient at the edge regimes of its split-K schedule (csrc/wgrad_x3.hip):
splits that own 1, 2 or 3 pixel tiles (the software pipelines' prologue / epilogue), the XCD-aware work-group order
with several (m, n) tiles, ragged and empty trailing splits, the 16+ -> multiple-of-8 rounding and the
512-work-group grid past 200 000 pixels — on wgrad_x3_kernel<3,3> / <2,2> / <1,1>, wgrad1_wide_kernel and
wgrad2_wide_kernel (tests/wgrad_x3_plan.py: REGIMES).  Each case asserts its regime through the launcher's own
plan (nps_conv2d_wgrad_x3_plan), then checks the weight gradient and the bias-gradient row of the same staging
against fp64.  A dropped or doubled pixel tile moves rel-L2 by >= sqrt(1 / ntiles) ~ 1.8e-2 in the largest case;
the bar is the project's fp32 one, 1e-5.
"""
import pytest
import torch

import wgrad_x3_plan as wp
from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
DB_TOL = 1e-6  # as test_wgrad_x3_bias_gradient_from_staging
DEV = "cuda"

# every regime at unit scale; one last-split-of-1 case and one 512-grid case again with tiny gradients x large
# activations, so the split-K partial atomics see the magnitudes of test_wgrad_x3_vs_fp64's range rows
CASES = [(case, want, 1.0, 1.0) for case, want in wp.REGIMES]
CASES += [(case, want, 1e-4, 1e3) for case, want in wp.REGIMES
          if case in ((1, 68, 68, 3, 1, 0, 75, 40), (2, 68, 68, 3, 1, 0, 320, 320))]
assert len(CASES) == len(wp.REGIMES) + 2


@pytest.mark.parametrize("case,want,sa,sx", CASES, ids=[f"{c}-{sa:g}-{sx:g}" for c, _, sa, sx in CASES])
def test_wgrad_schedule_vs_fp64(case, want, sa, sx):
    """G and db of one launch (ad.wgrad(..., db=db), db pre-filled with NaN) and G of a launch without the bias row
    against the fp64 gradient of the same fp32 inputs (a = randn * sa + 0.1 * sa, so the channel sums do not
    cancel); the fp32 CPU figures of the same sums are printed beside the kernel's.  Measured on MI355X: G 3.5e-7 ...
    9.3e-7 (fp32 CPU matmuls 8.5e-8 ... 2.1e-6), db 4.0e-8 ... 2.9e-7 (fp32 CPU sums 5.0e-8 ... 1.2e-7) — the
    204 800-pixel cases are the upper ends, so the existing 1e-6 bar of the bias row holds there as well."""
    from nps_hip import autograd as ad
    from nps_hip import ops
    B, M, N, k, pad, circ, Ha, Wa = case
    Hx, Wx = Ha + k - 1 - 2 * pad - 2 * circ, Wa + k - 1 - 2 * pad - 2 * circ
    # the regime this case is here for, from the launcher's own plan: kernel, remap, tiles of the last owning split
    # (and the rest of the row).  After a retune choose a new geometry with tests/wgrad_x3_plan.py.
    pl = wp.plan(*case)
    assert pl is not None and wp.regime(pl) == want, (case, pl, wp.regime(pl), want)
    assert ops.CONV_PRECISION == ops.PREC_X3F16 and ad.FUSE_DB  # (db from the kernels' staging, not a separate pass)
    torch.manual_seed(1)
    a = torch.randn(B, Ha, Wa, M) * sa + 0.1 * sa
    x = torch.randn(B, Hx, Wx, N) * sx
    ref = wp.ref_wgrad(a.double(), x.double(), k, pad, circ)
    ref_db = a.double().sum((0, 1, 2))
    ad_a, ad_x = a.to(DEV), x.to(DEV)
    db = torch.full((M,), float("nan"), device=DEV)
    g1 = ad.wgrad(ad_a, ad_x, k, k, pad=(pad, pad), circ=circ, db=db)
    g0 = ad.wgrad(ad_a, ad_x, k, k, pad=(pad, pad), circ=circ)
    e1, e0, edb = rel_l2(g1, ref), rel_l2(g0, ref), rel_l2(db, ref_db)
    e32 = rel_l2(wp.ref_wgrad(a, x, k, pad, circ), ref)  # fp32 CPU: the reference class
    edb32 = rel_l2(a.sum((0, 1, 2)), ref_db)
    print(f"wgrad schedule {case} x{sa:g} x{sx:g}: G {e1:.3e} / {e0:.3e} (fp32 CPU {e32:.3e}), "
          f"db {edb:.3e} (fp32 CPU {edb32:.3e})")
    assert e1 < TOL and e0 < TOL, (e1, e0, e32)
    assert edb < DB_TOL, (edb, edb32)
