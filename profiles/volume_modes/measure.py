"""Time the wrapper's volume-preservation step in each mode at the C3 shape -- B = 16, 3 fields, 256 x 256, time window
25 -- in one process: inference (two plane_sums, then nps_volume_rescale for 'individual_static', or nps_volume_factors
+ nps_volume_apply for 'block' / 'individual', in place on u) and training (the autograd Function's forward on a clone
plus its backward).  HIP events around INNER back-to-back calls, WARM warm-up rounds, the three modes alternating
within each of REPS rounds, medians and the min .. max spread per call.

Usage (on an MI355X, after build()):  python profiles/volume_modes/measure.py [OUT_DIR]
writes OUT_DIR/measure.json"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nps_hip import autograd as ad  # noqa: E402
from nps_hip import ops  # noqa: E402

DEV = "cuda"
B, C, TW, H, W = 16, 3, 25, 256, 256
M = 1.0 / 25.0
WARM, REPS, INNER = 3, 20, 10
MODES = ("individual_static", "block", "individual")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    g = torch.Generator().manual_seed(1)
    # totals close to the input's, as a trained model's are: every tanh regime costs the same, the values stay finite
    x = (0.25 + 0.5 * torch.rand(B, C, TW, H, W, generator=g)).to(DEV)
    u0 = (x + 0.01 * torch.randn(B, C, TW, H, W, generator=g).to(DEV)).contiguous()
    gy = torch.randn(B, C, TW, H, W, generator=g).to(DEV)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.9).float().to(DEV)
    tab = torch.from_numpy(np.cumsum(np.full(TW, np.float32(M), dtype=np.float32), dtype=np.float32)).to(DEV)
    u = u0.clone()

    def inference(mode):
        new_tot = ops.plane_sums(u, 0, H * W, H * W, B * C * TW)
        prev_tot = ops.plane_sums(x, (TW - 1) * H * W, TW * H * W, H * W, B * C)
        if mode == "individual_static":
            ops.volume_rescale(u, new_tot, prev_tot, tab, mask, 0)
        else:
            ops.volume_apply(u, ops.volume_factors(new_tot, prev_tot, mode, M, B, C, TW), mask, 0)

    def training(mode):
        ur = u0.detach().requires_grad_(True)
        if mode == "individual_static":
            y = ad.VolumeRescaleFn.apply(0, ur, x, tab, mask)
        else:
            y = ad.VolumeModeFn.apply((0, mode, M), ur, x, mask)
        y.backward(gy)

    res = dict(shape=[B, C, TW, H, W], max_pct_dif=M, warm=WARM, reps=REPS, inner=INNER,
               device=torch.cuda.get_device_name(0))
    for name, fn in (("inference", inference), ("training", training)):
        times = {m: [] for m in MODES}
        for r in range(WARM + REPS):
            for m in MODES:
                u.copy_(u0)  # in-place rescales compound otherwise; outside the timed window
                torch.cuda.synchronize()
                t = event_ms(lambda: fn(m))
                if r >= WARM:
                    times[m].append(t)
        res[name] = {m: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for m, v in times.items()}
        for m, v in res[name].items():
            print(f"{name:9s} {m:18s} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max {v['max_ms']:.4f})",
                  flush=True)
    assert torch.isfinite(u).all()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "measure.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
