"""Timing of the U-Net attention entry points against torch eager doing the same maths with the N x N scores
materialised (einsum -> softmax(dim=1) -> einsum, and its autograd backward), on the same fp32 inputs.

  python tools/attention_bench.py [--shapes B,N,heads,dk ...] [--skip-eager]

Per shape: HIP-event ms per call (3 warm-up calls, then a window of >= 0.5 s, alternating HIP / eager windows twice),
for  fwd = nps_attn_colstats + nps_attn_fwd  and  bwd = nps_attn_bwd  separately; the achieved share of the fp32
matrix peak (157.3 TFLOP/s) counts the tile GEMMs the kernels actually run — 3 of 2 N^2 dk FLOP per (batch, head)
forward (scores twice, P V once), 8 backward (key-tile kernel: scores, P^T dO, scores, dO V^T, dS^T Q; query-tile
kernel: scores, dO V^T, dS K) — against the algorithmic minimum of 2 and 4 that eager runs.  Also the rel-L2
difference of out and dqkv between the two.  One JSON line per shape.  Needs the GPU; reads nothing but its
arguments.  Each shape runs in a child process of its own under --timeout seconds; the first failure ends
the run."""
import argparse
import json
import math
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F32_MATRIX = 157.3e12


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, math.ceil(500.0 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def eager_fwd(qkv, heads, dk, scale):
    B, N = qkv.shape[:2]
    q, k, v = torch.chunk(qkv.view(B, N, heads, 3 * dk), 3, dim=-1)
    attn = (torch.einsum("bihd,bjhd->bijh", q, k) * scale).softmax(dim=1)
    return torch.einsum("bijh,bjhd->bihd", attn, v).reshape(B, N, heads * dk)


def rel(a, b):
    return (torch.linalg.vector_norm(a.double() - b.double()) / torch.linalg.vector_norm(b.double())).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["2,3481,1,192", "2,16129,1,192"])
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per shape")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:
        for spec in args.shapes:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", spec]
            rc = subprocess.run(cmd + (["--skip-eager"] if args.skip_eager else []), timeout=args.timeout).returncode
            if rc != 0:
                raise SystemExit(f"attention_bench: shape {spec} failed (exit status {rc})")
        return
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench: needs the GPU (no fallback)")
    from nps_hip import ops
    for spec in args.shapes:
        B, N, heads, dk = (int(v) for v in spec.split(","))
        scale = dk ** -0.5
        g = torch.Generator().manual_seed(N + dk)
        qkv = torch.randn(B, N, heads * 3 * dk, generator=g).cuda()
        dout = torch.randn(B, N, heads * dk, generator=g).cuda()
        out, lse = ops.attention(qkv, heads, dk, scale)
        dqkv = ops.attention_bwd(qkv, lse, dout, heads, dk, scale)
        res = dict(B=B, N=N, heads=heads, dk=dk)
        hip_f, hip_b, eag_f, eag_b = [], [], [], []
        qg = qkv.clone().requires_grad_(True)
        for _ in range(2):  # alternate the two implementations' windows
            hip_f.append(timed(lambda: ops.attention(qkv, heads, dk, scale)))
            hip_b.append(timed(lambda: ops.attention_bwd(qkv, lse, dout, heads, dk, scale)))
            if not args.skip_eager:
                with torch.no_grad():
                    eag_f.append(timed(lambda: eager_fwd(qkv, heads, dk, scale)))
                o = eager_fwd(qg, heads, dk, scale)
                eag_b.append(timed(lambda: torch.autograd.grad(o, qg, dout, retain_graph=True)))
                del o
        unit = 2.0 * B * heads * N * N * dk
        res.update(hip_fwd_ms=min(hip_f), hip_bwd_ms=min(hip_b), hip_fwd_ms_all=hip_f, hip_bwd_ms_all=hip_b,
                   hip_fwd_tflops_run=3 * unit / min(hip_f) / 1e9, hip_bwd_tflops_run=8 * unit / min(hip_b) / 1e9,
                   hip_fwd_peak_share=3 * unit / (min(hip_f) * 1e-3) / PEAK_F32_MATRIX,
                   hip_bwd_peak_share=8 * unit / (min(hip_b) * 1e-3) / PEAK_F32_MATRIX)
        if not args.skip_eager:
            with torch.no_grad():
                res["out_rel_l2_vs_eager"] = rel(out, eager_fwd(qkv, heads, dk, scale))
            o = eager_fwd(qg, heads, dk, scale)
            res["dqkv_rel_l2_vs_eager"] = rel(dqkv, torch.autograd.grad(o, qg, dout)[0])
            del o
            res.update(eager_fwd_ms=min(eag_f), eager_bwd_ms=min(eag_b), eager_fwd_ms_all=eag_f,
                       eager_bwd_ms_all=eag_b, fwd_speedup=min(eag_f) / min(hip_f), bwd_speedup=min(eag_b) / min(hip_b))
        print(json.dumps(res), flush=True)
        del qkv, dout, out, lse, dqkv, qg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
