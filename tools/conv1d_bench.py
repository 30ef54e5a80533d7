"""A/B timing of the 1-D U-Net convs on the MI355X: the Conv1d kernels (nps_conv1d_fwd) against stock PyTorch-ROCm
(F.conv1d / F.conv_transpose1d, fp32) per conv shape, and a 1-D UNetModern forward and training step on the HIP path
against the same module tree evaluated with torch's own ops.  The pointwise (K = 1) shapes get a third arm, the project's
own 2-D split-fp16 1x1 route on the (B, 1, L, C) view.

Workload (a choice: the reference ships no 1-D config): B = 16, L = 2048, UNetModern(num_spatial_dims=1,
hidden_features=128, n_cond=2, ch_mults=(1, 2, 2, 4), n_blocks=2, norm=True, padding_mode="ones"); the conv shapes are
those one inference forward of it launches.

Method: every shape and arm is warmed, then timed with device events around blocks of launches sized to ~0.15 s, the
arms alternating in both orders (A B B A ...), REPEATS blocks per arm (>= 0.5 s of work per arm); the record holds the
median per launch and the spread (max - min) / median of the blocks.

The training step needs every frame of the U-Net within the frame backward's limit of 4096 channels
(nps_frame_pack_bwd); at hidden_features = 128 the deepest up frame has 2048 + 2048 + 2 = 4098, so that arm is
recorded as not measured there and measured with --hidden 64 --only-e2e.

Usage:  python tools/conv1d_bench.py [--out profiles/conv1d/ab.jsonl] [--hidden 128] [--only-e2e] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

DEV = "cuda"
REPEATS = 4
BLOCK_S = 0.15


def _time_block(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def ab(arms, block_s=BLOCK_S, repeats=REPEATS):
    """arms: {name: fn}.  Returns {name: dict(median_us, spread, blocks_us)}."""
    names = list(arms)
    n = {}
    for k in names:
        for _ in range(3):
            arms[k]()
        torch.cuda.synchronize()
        t = _time_block(arms[k], 5)
        n[k] = max(3, int(block_s / max(t, 1e-7)))
    got = {k: [] for k in names}
    for r in range(repeats):
        for k in (names if r % 2 == 0 else names[::-1]):
            got[k].append(_time_block(arms[k], n[k]))
    return {k: dict(median_us=statistics.median(v) * 1e6, spread=(max(v) - min(v)) / statistics.median(v),
                    blocks_us=[round(t * 1e6, 2) for t in v], launches_per_block=n[k]) for k, v in got.items()}


# ------------------------------------------------------------------ the same module tree on torch's own ops
def _crop(x, L):
    from nps_hip import ops
    lo = ops.crop_offset(x.shape[-1], L)
    return F.pad(x, (lo, L - x.shape[-1] - lo))


def _conv(m, x):
    if isinstance(m, nn.ConvTranspose1d):
        return F.conv_transpose1d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)
    return F.conv1d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)


def _norm(m, x):
    return F.group_norm(x, m.num_groups, m.weight, m.bias, m.eps) if isinstance(m, nn.GroupNorm) else x


def _res(m, x):
    h = _conv(m.conv1, F.gelu(_norm(m.norm1, x)))
    h = _conv(m.conv2, F.gelu(_norm(m.norm2, h)))
    sc = x if isinstance(m.shortcut, nn.Identity) else _conv(m.shortcut, x)
    return _crop(h, sc.shape[-1]) + sc


def stock_unet(m, h, vb):
    """UNetModern.forward (no attention) with F.conv1d / F.group_norm / F.gelu / torch.cat on (B, C, L)."""
    from models.enc_proc_dec_components.proc_unet_modern import Downsample, Upsample
    L0 = h.shape[-1]
    feats, vbs = [h], [vb]
    for blk in m.down:
        if isinstance(blk, Downsample):
            h, vb = _conv(blk.conv, h), _conv(blk.conv_variables_broadcast, vb)
        else:
            h = _res(blk.res, torch.cat((h, vb), 1))
        feats.append(h)
        vbs.append(vb)
    h = _res(m.middle.res2, _res(m.middle.res1, torch.cat((h, vb), 1)))
    for blk in m.up:
        if isinstance(blk, Upsample):
            h = _conv(blk.conv, h)
        else:
            L = h.shape[-1]
            h = _res(blk.res, torch.cat((h, _crop(feats.pop(), L), _crop(vbs.pop(), L)), 1))
    return _crop(_conv(m.final, F.gelu(_norm(m.norm, h))), L0)


# ------------------------------------------------------------------ the benchmark
def conv_shapes(m, x, vb):
    """The distinct nps_conv1d_fwd launches of one inference forward: (Cin, Cout, K, stride, pad, L, out_os) -> count."""
    from nps_hip import ops
    seen, real = {}, ops.conv1d

    def spy(srcs, L, wpack, bias, Cout, K, stride=1, pad=(0, 0), out=None, out_os=1, **kw):
        cin = sum(s.t.shape[-1] for s in srcs)
        key = (cin, Cout, K, stride, tuple(pad), int(L), out_os)
        seen[key] = seen.get(key, 0) + 1
        return real(srcs, L, wpack, bias, Cout, K, stride=stride, pad=pad, out=out, out_os=out_os, **kw)

    ops.conv1d = spy
    try:
        with torch.no_grad():
            m(x, vb)
    finally:
        ops.conv1d = real
    return seen


def bench_shape(B, key):
    from nps_hip import ops
    cin, cout, K, stride, pad, L, out_os = key
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(B, L, cin, generator=g) * 2 - 1).to(DEV)
    xs = x.transpose(1, 2).contiguous()                       # the stock arm's own layout (B, C, L)
    flops_k = K if out_os == 1 else 4
    if out_os == 2:
        # the two 2-tap phases of one k4/s2 transposed conv (padding 1) against one F.conv_transpose1d
        w = (torch.rand(cin, cout, 4, generator=g) * 0.1).to(DEV)
        b = torch.zeros(cout, device=DEV)
        pk = [ops.pack_conv1d_weight(q) for q in ops.conv_transpose1d_phase_weights(w)]
        out = torch.empty(B, 2 * L, cout, device=DEV)

        def hip():
            for r in (0, 1):
                ops.conv1d([ops.Src1(x)], L, pk[r], b, cout, 2, pad=(1, 1), out=out, out_os=2, out_off=r - 1)

        stock = lambda: F.conv_transpose1d(xs, w, b, stride=2, padding=1)  # noqa: E731
        Lout = 2 * L
    else:
        w = (torch.rand(cout, cin, K, generator=g) * 0.1).to(DEV)
        b = torch.zeros(cout, device=DEV)
        pk = ops.pack_conv1d_weight(w)
        Lout = (L + pad[0] + pad[1] - K) // stride + 1
        out = torch.empty(B, Lout, cout, device=DEV)
        hip = lambda: ops.conv1d([ops.Src1(x)], L, pk, b, cout, K, stride=stride, pad=pad, out=out)  # noqa: E731
        stock = lambda: F.conv1d(xs, w, b, stride=stride, padding=pad[0])  # noqa: E731
    arms = dict(hip=hip, stock=stock)
    if K == 1 and out_os == 1:
        # a third arm for the pointwise shapes: the project's 2-D split-fp16 route, called as the U-Net's shortcut
        # would call it (one launch over the (1, L) image; sources off the 16-channel grid are frame-packed first)
        x4, pk2 = x.view(B, 1, L, cin), ops.pack_conv_weight(w.view(cout, cin, 1, 1))
        arms["route2d"] = lambda: ops.conv2d([ops.Src(x4)], (1, L), pk2, b, cout, 1, 1)  # noqa: E731
    res = ab(arms)
    nout = Lout if out_os == 1 else Lout // 2 * 2
    flops = 2.0 * B * nout * cout * cin * (flops_k if out_os == 1 else 2)
    nbytes = 4.0 * (B * L * cin + flops_k * cin * cout + B * nout * cout)
    rec = dict(kind="conv", B=B, L=L, cin=cin, cout=cout, K=K, stride=stride, pad=list(pad), out_os=out_os,
               flops=flops, bytes=nbytes, **{f"{k}_{f}": v[f] for k, v in res.items() for f in v})
    rec["hip_tflops"] = flops / (rec["hip_median_us"] * 1e-6) / 1e12
    rec["hip_gbs"] = nbytes / (rec["hip_median_us"] * 1e-6) / 1e9
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1d", "ab.jsonl"))
    ap.add_argument("--quick", action="store_true", help="B = 2, L = 256, hidden 32: a functional check of the tool")
    ap.add_argument("--hidden", type=int, default=128, help="hidden_features of the U-Net")
    ap.add_argument("--only-e2e", action="store_true", help="skip the per-shape arms")
    args = ap.parse_args()
    from models.enc_proc_dec_components import UNetModern
    B, L, hf = (2, 256, 32) if args.quick else (16, 2048, args.hidden)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(rec):
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(json.dumps(rec), flush=True)
    torch.manual_seed(0)
    m = UNetModern(pde=None, num_spatial_dims=1, n_cond=2, hidden_features=hf, ch_mults=(1, 2, 2, 4), n_blocks=2,
                   norm=True, padding_mode="ones", activation=nn.GELU()).to(DEV)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(B, hf, L, generator=g) * 2 - 1).to(DEV)
    vb = (torch.rand(B, 2, L, generator=g) * 2 - 1).to(DEV)
    with torch.no_grad():
        err = (m(x, vb) - stock_unet(m, x, vb)).norm() / stock_unet(m, x, vb).norm()
    print(f"U-Net forward, HIP path against torch ops: rel-L2 {err.item():.2e}", flush=True)
    for key, count in sorted(conv_shapes(m, x, vb).items() if not args.only_e2e else []):
        rec = bench_shape(B, key)
        rec["launches_per_forward"] = count
        emit(rec)

    def fwd_hip():
        with torch.no_grad():
            m(x, vb)

    def fwd_stock():
        with torch.no_grad():
            stock_unet(m, x, vb)

    gy = torch.rand(B, hf, L, generator=g).to(DEV)

    def step(fn):
        for p in m.parameters():
            p.grad = None
        (fn() * gy).sum().backward()

    for kind, arms in (("unet_forward", dict(hip=fwd_hip, stock=fwd_stock)),
                       ("unet_train_step", dict(hip=lambda: step(lambda: m(x, vb)),
                                                stock=lambda: step(lambda: stock_unet(m, x, vb))))):
        try:
            res = ab(arms, block_s=0.3)
        except RuntimeError as e:  # (a host check refused a launch: nothing ran)
            emit(dict(kind=kind, B=B, L=L, hidden_features=hf, not_measured=str(e)))
            continue
        emit(dict(kind=kind, B=B, L=L, hidden_features=hf, **{f"{k}_{f}": v[f] for k, v in res.items() for f in v}))
    out.close()


if __name__ == "__main__":
    main()
