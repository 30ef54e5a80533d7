"""Time one fp32 inference call of the 3-D FNO EncProcDec at the C5 volume, FNO.run alone on the same tensors, and
the pack / encoder / decoder alone.  HIP events, 5 warm-up calls, median of 30 repetitions.

Usage (on an MI355X, after build()):  python profiles/encprocdec_nd/measure.py [OUT_DIR]   -> OUT_DIR/measure.json"""
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

import models  # noqa: E402
from models.common import flat_frame  # noqa: E402
from nps_hip import ops  # noqa: E402

DEV = "cuda"
VOL, B, NUM_C, TW = (16, 128, 128), 1, 1, 25
CFG = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", processor="FNO", num_spatial_dims=3,
           num_c=NUM_C, time_window=TW, hidden_features=64, fno_modes=(8, 12, 12), hidden_blocks=4,
           cond_mode="concat", fno_kernel_size=1)
WARM, REPS = 5, 30


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    torch.manual_seed(0)
    pde = types.SimpleNamespace(dt=0.01, n_cond_static=4, n_cond_spatial=0)
    m = models.EncProcDec(pde=pde, activation=nn.GELU(), **CFG).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, NUM_C, TW, *VOL, generator=g).to(DEV)
    cond = torch.rand(B, 4, generator=g).to(DEV)
    axes = torch.meshgrid(*[torch.linspace(0, 1, s) for s in VOL], indexing="ij")
    pos = torch.stack(axes, dim=-1)[None].repeat(B, 1, 1, 1, 1).contiguous().to(DEV)
    N = VOL[0] * VOL[1] * VOL[2]
    CT, P, K, S = NUM_C * TW, 3, 4, 0
    Cp = (m.encoder.n_in + 3) // 4 * 4
    frame = (B,) + flat_frame(VOL)
    res = dict(device=torch.cuda.get_device_name(0), volume=VOL, B=B, cfg={k: str(v) for k, v in CFG.items()},
               warmup=WARM, reps=REPS)
    with torch.no_grad():
        res["model_call"] = timed(lambda: m(x, cond=cond, pos=pos))
        xin, vb = ops.pack_grid_input(x, pos, cond, None, Cp)
        xin4, vb4 = xin.view(frame + (Cp,)), vb.view(frame + (K + S,))
        h = m.encoder.run_packed(xin4, carry_stats=False)
        res["fno_run"] = timed(lambda: m.processor[0].run(h, vb4, D=VOL[0]))
        res["pack"] = timed(lambda: ops.pack_grid_input(x, pos, cond, None, Cp))
        res["encoder"] = timed(lambda: m.encoder.run_packed(xin4, carry_stats=False))
        hp = m.processor[0].run(h, vb4, D=VOL[0])
        res["decoder"] = timed(lambda: m.decoder.run(hp, x))
    nbytes = 4 * B * N * (CT + P + S + Cp + K + S)
    res["pack"]["algorithmic_bytes"] = nbytes
    res["pack"]["achieved_GBps"] = nbytes / (res["pack"]["median_ms"] * 1e-3) / 1e9
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "measure.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
