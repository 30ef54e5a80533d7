"""A/B timing of SpectralConv2d for a caller holding NCHW tensors (default: the C3 FNO-layer shape, B=16, 256x256,
196 -> 192 channels, 10 modes), forward and backward separately, HIP-event time per call over a window >= 0.5 s.

  --arm A  what such a caller had to do before the channels-first entry points: nps_nchw_to_nhwc ->
           nps_spectral_conv2d_fwd -> nps_nhwc_to_nchw (backward: x and dy in, dx out, around nps_spectral_conv2d_bwd).
           Also prints the pure NHWC call without the transposes, as context.
  --arm B  nps_spectral_conv2d_fwd_nchw / _bwd_nchw on the same NCHW tensors, plus the two channels-first W passes
           alone with their algorithmic bytes (inputs read once + outputs written once).
           With --compare-lib LIB it also runs arm A's route from LIB on the same inputs and prints the rel-L2
           difference of y, dx, dw1.

Bare ctypes on --lib (no nps_hip import), so arm A can load a library built from an older commit.  One JSON line."""
import argparse
import ctypes
import json
import math

import torch

VP, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


def load(path, nchw):
    lib = ctypes.CDLL(path)
    sigs = {
        "nps_nchw_to_nhwc": [VP, VP, I, I, I, I, VP],
        "nps_nhwc_to_nchw": [VP, VP, I, I, I, I, VP],
        "nps_spectral_conv2d_fwd": [VP] * 5 + [I] * 9 + [VP],
        "nps_spectral_conv2d_bwd": [VP] * 8 + [I] * 7 + [VP],
    }
    if nchw:
        sigs.update({
            "nps_spectral_conv2d_fwd_nchw": [VP, L, VP, VP, VP, L, VP] + [I] * 9 + [VP],
            "nps_spectral_conv2d_bwd_nchw": [VP, L, VP, VP, VP, L, VP, L, VP, VP, VP] + [I] * 7 + [VP],
            "nps_spectral_dft_w_nchw": [VP, L, I, I, I, I, I, VP, VP],
            "nps_spectral_idft_w_nchw": [VP, VP, L, I, I, I, I, I, I, I, VP],
        })
    for n, a in sigs.items():
        f = getattr(lib, n)
        f.restype, f.argtypes = I, a
    lib.nps_spectral_conv2d_workspace.restype, lib.nps_spectral_conv2d_workspace.argtypes = ctypes.c_size_t, [I] * 7
    lib.nps_last_error.restype = ctypes.c_char_p
    return lib


def timed(fn, lib, what):
    """Mean HIP-event ms per call: 3 warm-up calls, then enough repetitions for a window of at least 0.5 s."""
    for _ in range(3):
        rc = fn()
        if rc != 0:
            raise RuntimeError(f"{what}: rc {rc}: {lib.nps_last_error().decode()}")
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
    return e0.elapsed_time(e1) / reps, reps


def rel_l2(a, b):
    a, b = torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b
    return (torch.linalg.vector_norm((a - b).double()) / torch.linalg.vector_norm(b.double())).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--arm", choices=["A", "B"], required=True)
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--cin", type=int, default=196)
    ap.add_argument("--cout", type=int, default=192)
    ap.add_argument("--m", type=int, default=10)
    args = ap.parse_args()
    B, H, W, Ci, Co, m = args.b, args.hw, args.hw, args.cin, args.cout, args.m
    dev = "cuda"
    torch.manual_seed(0)
    c64 = torch.complex64
    x = torch.randn(B, Ci, H, W, device=dev)
    dy = torch.randn(B, Co, H, W, device=dev)
    w1 = torch.rand(Ci, Co, m, m, dtype=c64, device=dev) / (Ci * Co)
    w2 = torch.rand(Ci, Co, m, m, dtype=c64, device=dev) / (Ci * Co)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    s = VP(torch.cuda.current_stream().cuda_stream)
    p = lambda t: VP(t.data_ptr())  # noqa: E731
    dims = (B, Ci, Co, H, W, m, m)
    res = {"arm": args.arm, "label": args.label, "lib": args.lib, "shape": [B, Ci, Co, H, W, m],
           "device": torch.cuda.get_device_name(0)}

    def route_a(lib):
        """The NHWC composites between layout transposes; returns the forward / backward closures."""
        ws = torch.empty(lib.nps_spectral_conv2d_workspace(*dims), dtype=torch.uint8, device=dev)
        xt, dxt = torch.empty(B, H, W, Ci, device=dev), torch.empty(B, H, W, Ci, device=dev)
        yt, dyt = torch.empty(B, H, W, Co, device=dev), torch.empty(B, H, W, Co, device=dev)

        def fwd_pure():
            return lib.nps_spectral_conv2d_fwd(p(xt), p(w1), p(w2), p(yt), p(ws), *dims, 0, 0, s)

        def bwd_pure():
            return lib.nps_spectral_conv2d_bwd(p(xt), p(w1), p(w2), p(dyt), p(dxt), p(dw1), p(dw2), p(ws), *dims, s)

        def fwd():
            return (lib.nps_nchw_to_nhwc(p(x), p(xt), B, Ci, H, W, s) or fwd_pure()
                    or lib.nps_nhwc_to_nchw(p(yt), p(y), B, Co, H, W, s))

        def bwd():
            return (lib.nps_nchw_to_nhwc(p(x), p(xt), B, Ci, H, W, s)
                    or lib.nps_nchw_to_nhwc(p(dy), p(dyt), B, Co, H, W, s) or bwd_pure()
                    or lib.nps_nhwc_to_nchw(p(dxt), p(dx), B, Ci, H, W, s))
        return fwd, bwd, fwd_pure, bwd_pure, (ws, xt, dxt, yt, dyt)

    if args.arm == "A":
        lib = load(args.lib, nchw=False)
        fwd, bwd, fwd_pure, bwd_pure, _keep = route_a(lib)
        res["fwd_ms"], res["fwd_reps"] = timed(fwd, lib, "A fwd")
        res["bwd_ms"], res["bwd_reps"] = timed(bwd, lib, "A bwd")
        res["fwd_nhwc_only_ms"], _ = timed(fwd_pure, lib, "A fwd (no transposes)")
        res["bwd_nhwc_only_ms"], _ = timed(bwd_pure, lib, "A bwd (no transposes)")
    else:
        lib = load(args.lib, nchw=True)
        ws = torch.empty(lib.nps_spectral_conv2d_workspace(*dims), dtype=torch.uint8, device=dev)

        def fwd():
            return lib.nps_spectral_conv2d_fwd_nchw(p(x), 0, p(w1), p(w2), p(y), 0, p(ws), *dims, 0, 0, s)

        def bwd():
            return lib.nps_spectral_conv2d_bwd_nchw(p(x), 0, p(w1), p(w2), p(dy), 0, p(dx), 0, p(dw1), p(dw2), p(ws),
                                                    *dims, s)
        res["fwd_ms"], res["fwd_reps"] = timed(fwd, lib, "B fwd")
        res["bwd_ms"], res["bwd_reps"] = timed(bwd, lib, "B bwd")
        X1 = torch.empty(B, H, m, Ci, dtype=c64, device=dev)
        Z = torch.randn(B, H, m, Co, dtype=c64, device=dev)
        ms, _ = timed(lambda: lib.nps_spectral_dft_w_nchw(p(x), 0, B, H, W, Ci, m, p(X1), s), lib, "dft_w_nchw")
        nb = x.numel() * 4 + X1.numel() * 8
        res["dft_w_nchw"] = {"ms": ms, "bytes": nb, "TBps": nb / (ms * 1e-3) / 1e12}
        ms, _ = timed(lambda: lib.nps_spectral_idft_w_nchw(p(Z), p(y), 0, B, H, W, m, Co, 0, 0, s), lib, "idft_w_nchw")
        nb = Z.numel() * 8 + y.numel() * 4
        res["idft_w_nchw"] = {"ms": ms, "bytes": nb, "TBps": nb / (ms * 1e-3) / 1e12}
        if args.compare_lib:
            assert fwd() == 0 and bwd() == 0
            torch.cuda.synchronize()
            yb, dxb, dw1b = y.clone(), dx.clone(), dw1.clone()
            y.fill_(float("nan")), dx.fill_(float("nan")), dw1.fill_(float("nan"))
            liba = load(args.compare_lib, nchw=False)
            fa, ba, _, _, _keep = route_a(liba)
            assert fa() == 0 and ba() == 0
            torch.cuda.synchronize()
            res["vs_A"] = {"lib": args.compare_lib, "y_rel_l2": rel_l2(yb, y), "dx_rel_l2": rel_l2(dxb, dx),
                           "dw1_rel_l2": rel_l2(dw1b, dw1), "y_bit_identical": bool(torch.equal(yb, y)),
                           "dx_bit_identical": bool(torch.equal(dxb, dx))}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
