"""Times nps_conv3d_fwd (fp32), the input-gradient launch(es) and nps_conv3d_wgrad at the 3-D U-Net conv shapes of
bench.py's C5_UFNO_CFG (read off one no-grad forward of the first block's U-Net, B = 1)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")]
import torch  # noqa: E402
from nps_hip import ops, autograd as ad  # noqa: E402
from bench import C5_UFNO_CFG, C5_VOL, C5_CFG  # noqa: E402
from models.enc_proc_dec_components.proc_ufno import UFNO  # noqa: E402

DEV = "cuda"
PEAK = 157.3e12
torch.manual_seed(0)
m = UFNO(pde=None, **dict(C5_UFNO_CFG, hidden_blocks=1)).to(DEV).eval()
D, H, W = C5_VOL
B = 1
shapes = []
_conv3d = ops.conv3d


def spy(srcs, frame_dhw, wpack, bias, Cout, K, stride=1, transposed=False, circ=0, zpad=0, **kw):
    shapes.append(dict(cin=sum(s.t.shape[4] for s in srcs), cout=Cout, K=K, stride=stride, transposed=bool(transposed),
                       dhw=tuple(int(v) for v in frame_dhw), circ=circ, zpad=zpad))
    return _conv3d(srcs, frame_dhw, wpack, bias, Cout, K, stride=stride, transposed=transposed, circ=circ, zpad=zpad,
                   **kw)


ops.conv3d = spy
with torch.no_grad():
    m.run3d(torch.rand(B, D, H, W, C5_CFG["hidden_features"], device=DEV),
            torch.rand(B, D, H, W, C5_CFG["n_cond"], device=DEV))
ops.conv3d = _conv3d
torch.cuda.synchronize()
for s in shapes:
    print("shape", json.dumps(s), flush=True)


def pick(pred):
    return next(s for s in shapes if pred(s))


def timed(fn, iters=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def report(name, what, ms, flops):
    tf = flops / (ms * 1e-3) / 1e12
    row = dict(layer=name, launch=what, ms=round(ms, 4), TFs=round(tf, 2), frac_peak=round(tf * 1e12 / PEAK, 4))
    print("time", json.dumps(row), flush=True)
    return ms


def conv_case(name, s):
    K, st, cin, cout = s["K"], s["stride"], s["cin"], s["cout"]
    x = torch.randn(B, *s["dhw"], cin, device=DEV)
    w = torch.nn.Parameter(torch.randn(cout, cin, K, K, K, device=DEV) * 0.05)
    wp = ops.pack_conv3d_weight(w)
    # the conv kernel alone: the frame as the product path hands it over (channels padded to 16, one source)
    xq = x if cin % 16 == 0 else ops.frame_pack3d([ops.Src3(x)], s["dhw"])
    y = ops.conv3d([ops.Src3(xq)], s["dhw"], wp, None, cout, K, stride=st, circ=s["circ"], zpad=s["zpad"])
    gy = torch.randn_like(y)
    flops = 2.0 * y.numel() * cin * K ** 3
    f = report(name, "fwd", timed(lambda: ops.conv3d([ops.Src3(xq)], s["dhw"], wp, None, cout, K, stride=st,
                                                     circ=s["circ"], zpad=s["zpad"])), flops)
    if st == 1:
        wd = ops.pack_conv3d_weight(ops.conv3d_dgrad_weight(w))
        zp = 0 if s["circ"] else K - 1 - s["zpad"]
        report(name, "dgrad", timed(lambda: ops.conv3d([ops.Src3(gy)], gy.shape[1:4], wd, None, cin, K, circ=s["circ"],
                                                       zpad=zp)), flops)
    else:
        wt = ops.pack_conv3d_weight(ops.conv3d_s2_dgrad_weight(w), transposed=True)
        dx = torch.empty_like(x)
        z = s["zpad"]
        report(name, "dgrad", timed(lambda: ops.conv3d([ops.Src3(gy)], gy.shape[1:4], wt, None, cin, 2, transposed=True,
                                                       zpad=1, out=dx, out_os=2, out_off=(-z,) * 3)), flops)
    g = torch.zeros(cout, cin, K, K, K, device=DEV)
    wg = report(name, "wgrad", timed(lambda: ops.conv3d_wgrad(gy, x, K, stride=st, circ=s["circ"], zpad=s["zpad"],
                                                              g=g)), flops)
    print("ratio", json.dumps(dict(layer=name, wgrad_over_fwd=round(wg / f, 3),
                                   splits=ops.conv3d_wgrad_splits(gy, x, K, st, s["circ"], s["zpad"]))), flush=True)


def up_case(name, s):
    cin, cout, c = s["cin"], s["cout"], s["circ"]
    x = torch.randn(B, *s["dhw"], cin, device=DEV)
    w = torch.nn.Parameter(torch.randn(cin, cout, 4, 4, 4, device=DEV) * 0.05)
    wp = ops.pack_conv3d_weight(w, transposed=True)

    def fwd():
        return ops.conv3d([ops.Src3(x)], s["dhw"], wp, None, cout, 2, transposed=True, circ=c, zpad=1)
    y = fwd()
    gy = torch.randn_like(y)
    Dp, Hp, Wp = (n + 2 * c for n in s["dhw"])
    flops = 2.0 * B * Dp * Hp * Wp * cin * cout * 64
    f = report(name, "fwd", timed(fwd), flops)
    wd = ops.pack_conv3d_weight(ops.conv_transpose3d_dgrad_weight(w))
    dq = ops.space_to_depth3d(gy, Dp + 1, Hp + 1, Wp + 1)
    report(name, "dgrad: space_to_depth3d", timed(lambda: ops.space_to_depth3d(gy, Dp + 1, Hp + 1, Wp + 1)), 0.0)
    report(name, "dgrad: K=2 conv", timed(lambda: ops.conv3d([ops.Src3(dq)], dq.shape[1:4], wd, None, cin, 2)), flops)
    dxp = ops.conv3d([ops.Src3(dq)], dq.shape[1:4], wd, None, cin, 2)
    report(name, "dgrad: circular_fold3d", timed(lambda: ops.circular_fold3d(dxp, c)), 0.0)
    xp = ops.circular_pad3d(x, c)
    report(name, "wgrad: circular_pad3d", timed(lambda: ops.circular_pad3d(x, c)), 0.0)
    g = torch.zeros(cin, cout, 4, 4, 4, device=DEV)
    wg = report(name, "wgrad", timed(lambda: ops.conv3d_wgrad(xp, gy, 4, stride=2, g=g)), flops)
    print("ratio", json.dumps(dict(layer=name, wgrad_over_fwd=round(wg / f, 3),
                                   splits=ops.conv3d_wgrad_splits(xp, gy, 4, 2))), flush=True)


conv_case("conv 68->64 K3 valid", pick(lambda s: s["K"] == 3 and s["stride"] == 1 and s["cin"] == 68))
conv_case("Downsample K3 s2", pick(lambda s: s["K"] == 3 and s["stride"] == 2 and s["cin"] == 64))
up_case("Upsample k4 s2", pick(lambda s: s["transposed"]))
