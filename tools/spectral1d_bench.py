"""A/B timing of SpectralConv1d on (B, C, L) tensors: the HIP path (models' SpectralConv1d: layout kernels, L-split
truncated DFTs, the shared mixer) against what a user runs today on the same GPU in stock PyTorch-ROCm, the
reference's own route torch.fft.rfft -> einsum -> torch.fft.irfft with autograd (restated below).

Both arms run in one process, alternating, --reps times each (default 3): forward (no_grad) and forward+backward
(gradients of x and weights1), HIP-event time per call, 3 warm-ups then a window of at least 0.5 s.  Reports the
medians and the spread, the rel-L2 of y, dx and dW between the arms at the timed shape, and each new kernel alone
with its algorithmic bytes (inputs read once + outputs written once; the tensors are largely cache-resident, so the
bytes/s are context against the HBM peak, not a gate).  One JSON line per run.

  python tools/spectral1d_bench.py --b 16 --c 128 --l 1024 --m 48
  python tools/spectral1d_bench.py --b 64 --c 64 --l 4096 --m 32
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402


class TorchSpectralConv1d(nn.Module):
    """The stock route: rfft, per-mode complex einsum on the first m bins, zero-padded irfft."""

    def __init__(self, weights1):
        super().__init__()
        self.weights1 = nn.Parameter(weights1.detach().clone())

    def forward(self, x):
        B, _, L = x.shape
        Cout, m = self.weights1.shape[1], self.weights1.shape[2]
        x_ft = torch.fft.rfft(x)
        out_ft = torch.zeros(B, Cout, L // 2 + 1, device=x.device, dtype=torch.complex64)
        out_ft[:, :, :m] = torch.einsum("bix,iox->box", x_ft[:, :, :m], self.weights1)
        return torch.fft.irfft(out_ft, n=L)


def timed(fn):
    """Mean HIP-event ms per call: 3 warm-up calls, then enough repetitions for a window of at least 0.5 s."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, math.ceil(600.0 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rel_l2(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return (torch.linalg.vector_norm((a - b).double()) / torch.linalg.vector_norm(b.double())).item()


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--c", type=int, default=128)
    ap.add_argument("--l", type=int, default=1024)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    B, C, L, m = args.b, args.c, args.l, args.m
    import nps_hip
    from nps_hip import ops
    from models.enc_proc_dec_components.proc_fno import SpectralConv1d
    dev = "cuda"
    torch.manual_seed(0)
    hip = SpectralConv1d(C, C, (m,)).to(dev)
    ref = TorchSpectralConv1d(hip.weights1).to(dev)
    x = torch.randn(B, C, L, device=dev, requires_grad=True)
    g = torch.randn(B, C, L, device=dev)
    res = {"label": args.label, "shape": {"B": B, "C": C, "L": L, "m": m}, "device": torch.cuda.get_device_name(0),
           "reps": args.reps}

    def fwd(mod):
        def run():
            with torch.no_grad():
                return mod(x)
        return run

    def fwd_bwd(mod):
        def run():
            x.grad = None
            mod.weights1.grad = None
            y = mod(x)
            y.backward(g)
            return y
        return run

    # the two arms agree at the timed shape
    y_h = fwd_bwd(hip)().detach().clone()
    dx_h, dw_h = x.grad.clone(), hip.weights1.grad.clone()
    y_t = fwd_bwd(ref)().detach().clone()
    res["hip_vs_torch_rel_l2"] = {"y": rel_l2(y_h, y_t), "dx": rel_l2(dx_h, x.grad), "dW": rel_l2(dw_h, ref.weights1.grad)}

    t = {k: [] for k in ("hip_fwd", "torch_fwd", "hip_fwd_bwd", "torch_fwd_bwd")}
    for _ in range(args.reps):  # alternating arms
        t["hip_fwd"].append(timed(fwd(hip)))
        t["torch_fwd"].append(timed(fwd(ref)))
        t["hip_fwd_bwd"].append(timed(fwd_bwd(hip)))
        t["torch_fwd_bwd"].append(timed(fwd_bwd(ref)))
    for k, v in t.items():
        res[k] = summary(v)
    res["hip_not_slower"] = {"fwd": res["hip_fwd"]["median_ms"] <= res["torch_fwd"]["median_ms"],
                             "fwd_bwd": res["hip_fwd_bwd"]["median_ms"] <= res["torch_fwd_bwd"]["median_ms"]}

    # each new kernel alone, channels-last (B, L, C)
    lib, s = nps_hip.lib, nps_hip.stream_ptr()
    p = lambda a: a.data_ptr()  # noqa: E731
    c64 = torch.complex64
    xl = torch.randn(B, L, C, device=dev)
    X = torch.empty(B, m, C, dtype=c64, device=dev)
    Z = torch.randn(B, m, C, dtype=c64, device=dev)
    yl = torch.empty(B, L, C, device=dev)
    ws = torch.empty(max(lib.nps_spectral1d_dft_workspace(B, L, C, m), 4), dtype=torch.uint8, device=dev)
    src = ops._c_src([ops.Src(xl.unsqueeze(1))])

    def kernel(name, fn, nbytes):
        assert fn() == 0, lib.nps_last_error()
        ms = timed(fn)
        res[name] = {"ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12}

    io = xl.numel() * 4 + X.numel() * 8
    kernel("dft", lambda: lib.nps_spectral1d_dft(src, 1, B, L, C, m, p(X), p(ws), 0, s), io)
    kernel("dft_adjoint", lambda: lib.nps_spectral1d_dft(src, 1, B, L, C, m, p(X), p(ws), 1, s), io)
    kernel("idft", lambda: lib.nps_spectral1d_idft(p(Z), p(yl), B, L, m, C, 0, None, 0, 0, s), io)
    kernel("idft_accumulate_gelu", lambda: lib.nps_spectral1d_idft(p(Z), p(yl), B, L, m, C, 1, None, 1, 0, s),
           io + yl.numel() * 4)
    kernel("idft_adjoint", lambda: lib.nps_spectral1d_idft(p(Z), p(yl), B, L, m, C, 0, None, 0, 1, s), io)
    wp = torch.zeros(m, C, C, dtype=c64, device=dev)
    Y = torch.empty(B, m, C, dtype=c64, device=dev)
    kernel("mix", lambda: lib.nps_spectral_mix(p(X), p(wp), p(Y), B, 1, m, C, C, s),
           X.numel() * 8 + wp.numel() * 8 + Y.numel() * 8)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
