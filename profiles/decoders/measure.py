"""Time the three decoders that run on the decode-chain kernel (dec_grid.TimeConvLinear, TimeConv, LinearConv) at the
cfgs' shape -- B = 16, 256 x 256, num_c = 3, tw = 25, hidden 128 -- forward (no grad) and forward + backward, and the
same chain composed from stock PyTorch-ROCm ops (tests/decoders_ref.py in fp32 on the same device: the reference's own
op sequence).  Both sides take h as (B, hidden, H, W); `run` is the HIP decoder on the channels-last h that EncProcDec
hands it (no layout transposes).  One process times one side of one decoder (a first call can spend minutes choosing a
stock convolution algorithm: each side gets a time limit of its own from the caller); HIP events, WARM warm-up calls,
the variants alternating within each of REPS rounds, medians.  The first call's wall time is reported apart.

Usage (on an MI355X, after build()):  python profiles/decoders/measure.py CASE hip|stock [OUT_DIR]
appends one JSON line to OUT_DIR/measure.jsonl"""
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

import decoders_ref as R  # noqa: E402
from models.enc_proc_dec_components import dec_grid  # noqa: E402
from nps_hip import ops  # noqa: E402

DEV = "cuda"
B, H, W, NUM_C, TW, HIDDEN, DT = 16, 256, 256, 3, 25, 128, 0.01
WARM, REPS = 3, 10
BASE = dict(num_c=NUM_C, num_spatial_dims=2, time_window=TW, hidden_features=HIDDEN)
CASES = {
    "TimeConvLinear": dict(BASE),
    "TimeConv": dict(BASE),
    "LinearConv": dict(BASE, dec_kernel_size=3, dec_padding_mode="circular"),
}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def say(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, flush=True)


def main():
    cls, side = sys.argv[1], sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.dirname(os.path.abspath(__file__))
    kw = CASES[cls]
    g = torch.Generator().manual_seed(1)
    h = torch.randn(B, HIDDEN, H, W, generator=g).to(DEV)
    u = torch.rand(B, NUM_C, TW, H, W, generator=g).to(DEV)
    gy = torch.randn(B, NUM_C, TW, H, W, generator=g).to(DEV)
    torch.manual_seed(0)
    extra = {} if cls in ("TimeConv", "LinearConv") else dict(activation=nn.GELU())
    m = getattr(dec_grid, cls)(pde=types.SimpleNamespace(dt=DT), **kw, **extra).to(DEV)
    rec = dict(case=cls, side=side, device=torch.cuda.get_device_name(0), warmup=WARM, reps=REPS,
               shape=dict(B=B, H=H, W=W, num_c=NUM_C, tw=TW, hidden=HIDDEN))
    if side == "hip":
        h_cl = ops.nchw_to_nhwc(h)

        def fwd():
            with torch.no_grad():
                m(h, u)

        def run():
            with torch.no_grad():
                m.run(h_cl, u)

        def fwd_bwd():
            hh = h.detach().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            m(hh, u).backward(gy)
        variants = dict(fwd=fwd, run=run, fwd_bwd=fwd_bwd)
    else:
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}

        def fwd():
            with torch.no_grad():
                R.decoder(cls, sd, h, u, DT, kw)

        def fwd_bwd():
            hh = h.detach().requires_grad_(True)
            for v in sd.values():
                v.grad = None
            R.decoder(cls, sd, hh, u, DT, kw).backward(gy)
        variants = dict(fwd=fwd, fwd_bwd=fwd_bwd)
    first = {}
    for k, fn in variants.items():
        say(f"{cls} {side}: first {k} ...")
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        first[k] = time.time() - t0
        say(f"{cls} {side}: first {k} took {first[k]:.2f} s")
    rec["first_call_s"] = first
    if side == "stock":
        with torch.no_grad():
            y_hip, y_stock = m(h, u), R.decoder(cls, sd, h, u, DT, kw)
        rec["hip_vs_stock_rel_l2"] = (torch.linalg.vector_norm(y_hip.double() - y_stock.double()) /
                                      torch.linalg.vector_norm(y_stock.double())).item()
    times = {k: [] for k in variants}
    for r in range(WARM + REPS):
        for k, fn in variants.items():
            t = event_ms(fn)
            if r >= WARM:
                times[k].append(t)
    for k, v in times.items():
        rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    say(json.dumps(rec))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "measure.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
