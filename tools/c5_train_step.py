"""One forward + backward of the C5 3-D U-FNO (bench.C5_UFNO_CFG, fp32, B = 1) on the 16 x 128 x 128 volume.
--steps N --warmup W: steady-state time per step (device events around each step, after W warm-up steps), the peak
memory, and the bytes nps_frame3d_bwd's two passes must move per step, counted from the shapes of every call
(pass 1: gy + the covered source voxels; pass 2: per source the covered voxels of the source, gy and gy_plain read,
the whole source gradient written).  For kernel times run it under `rocprofv3 --kernel-trace --stats` in a run of
its own (profiles/unet3d_train/README.md).  --vol D H W: another volume."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")):
    sys.path.insert(0, p)
os.environ.setdefault("NPS_AUTO_DIST", "0")
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--vol", type=int, nargs=3, default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

from bench import C5_UFNO_CFG, C5_CFG, C5_VOL  # noqa: E402
from models.enc_proc_dec_components.proc_ufno import UFNO  # noqa: E402
from nps_hip import ops  # noqa: E402

dev = "cuda"
torch.manual_seed(42)
m = UFNO(pde=None, **C5_UFNO_CFG).to(dev)
D, H, W = args.vol or C5_VOL
g = torch.Generator(device=dev).manual_seed(1234)
h = (torch.rand(1, C5_CFG["hidden_features"], D, H, W, device=dev, generator=g) * 2 - 1).requires_grad_(True)
vb = torch.rand(1, C5_CFG["n_cond"], D, H, W, device=dev, generator=g)
gy = torch.randn(1, C5_CFG["hidden_features"], D, H, W, device=dev, generator=g)

count = {"p1": 0, "p2": 0, "calls": 0, "gn_calls": 0}
_orig = ops.frame3d_bwd


def counted(srcs, frame_dhw, gn, pre_act, gy_, gy_plain=None, need=None):
    nvox = frame_dhw[0] * frame_dhw[1] * frame_dhw[2]
    cin = sum(s.t.shape[4] for s in srcs)
    cov = []
    for s in srcs:
        n = 1
        for o, sz, f in zip((s.off_d, s.off_h, s.off_w), s.t.shape[1:4], frame_dhw):
            n *= max(0, min(f, o + sz) - max(0, o))
        cov.append(n)
    B = srcs[0].t.shape[0]
    count["calls"] += 1
    if gn is not None:
        count["gn_calls"] += 1
        count["p1"] += 4 * B * (nvox * cin + sum(c * s.t.shape[4] for c, s in zip(cov, srcs)))
    for i, (c, s) in enumerate(zip(cov, srcs)):
        if need is None or need[i]:
            C = s.t.shape[4]
            count["p2"] += 4 * B * (c * C * (2 + (gy_plain is not None)) + s.t[0].numel())
    return _orig(srcs, frame_dhw, gn, pre_act, gy_, gy_plain, need)


ops.frame3d_bwd = counted


def step():
    for p in m.parameters():
        p.grad = None
    h.grad = None
    y = m(h, variables_broadcast=vb)
    (y * gy).sum().backward()
    return y


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
for k in count:
    count[k] = 0
times = []
t0 = time.perf_counter()
for _ in range(args.steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
wall = time.perf_counter() - t0
times.sort()
res = dict(volume=[D, H, W], steps=args.steps, warmup=args.warmup, ms_median=times[len(times) // 2], ms_min=times[0],
           ms_max=times[-1], wall_s=wall, peak_mem_GiB=torch.cuda.max_memory_allocated() / 2 ** 30,
           frame3d_bwd_calls_per_step=count["calls"] / args.steps, gn_calls_per_step=count["gn_calls"] / args.steps,
           pass1_bytes_per_step=count["p1"] / args.steps, pass2_bytes_per_step=count["p2"] / args.steps,
           grads_finite=all(torch.isfinite(torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).all().item()
                            for p in m.parameters()))
print(json.dumps(res), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f)
