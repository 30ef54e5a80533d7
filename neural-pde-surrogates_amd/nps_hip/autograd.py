"""Differentiable front end of the HIP kernels (the training / backward hot path).

Each `torch.autograd.Function` below runs its forward AND backward through
libnps_hip.so: convs (input gradients as forward convs of dy with re-packed
weights, weight gradients on the MFMA wgrad kernel), the GroupNorm+GELU frame
backward, SpectralConv2d backward, the TimeConvDense decoder and the
activation_wrapper volume rescale.  Tensors are NHWC fp32 on the MI355X; no op
falls back to a CPU or aten compute path.  PyTorch supplies autograd's graph,
memory (clone / zeros) and gradient accumulation only.

Reference semantics: trainers/base.py:492 `loss.backward()` over the modules of
models/ (see each Function's docstring for the op it differentiates).
"""
import ctypes
import os
from typing import List, Optional, Sequence

import torch

from . import Conv2dArgs, WgradArgs, check, lib, ptr, stream_ptr
from . import ops
from .ops import Src

GELU = ops.GELU


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------- weight gradient
def wgrad(a: torch.Tensor, x: torch.Tensor, KH: int, KW: int, dil=1, pad=(0, 0), circ=0,
          g: Optional[torch.Tensor] = None, a_range: Optional[int] = None, x_range: Optional[int] = None,
          db: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G[m][n][KH*KW] (+)= sum_pix a[pix][m] * Xext[pix + tap*dil - pad][n].

    Split-fp16 MFMA (nps_conv2d_wgrad_x3) under ops.CONV_PRECISION == PREC_X3F16 for undilated square
    kernels up to 3x3 over channel counts that are multiples of 4 — a and x range-scaled from their
    max |.| (a_range / x_range: a's / x's range-tag pointers when the caller already has them) — else exact fp32 MFMA
    (nps_conv2d_wgrad).  db ([M], with g is None): also db[m] = sum_pix a[pix][m] (the conv's bias gradient when
    a = dy) — from the split-fp16 kernels' own staging of a (nps_wgrad_t.db), else an nps_channel_sums pass."""
    a, x = _c(a), _c(x)
    B, Ha, Wa, M = a.shape
    _, Hx, Wx, N = x.shape
    x3 = ops.CONV_PRECISION == ops.PREC_X3F16 and KH == KW and KH <= 3 and dil == 1
    store = g is None and x3 and M % 4 == 0 and N % 4 == 0  # the split-fp16 fold stores g: no zero-fill
    if db is not None and not (store and FUSE_DB):
        db.zero_()
        check(lib.nps_channel_sums(ptr(a), a.numel() // M, M, ptr(db), stream_ptr()), "channel_sums")
        db = None
    if g is None:
        g = (torch.empty if store else torch.zeros)((M, N, KH, KW), dtype=torch.float32, device=a.device)
    if (ops.CONV_PRECISION == ops.PREC_X3F16 and KH == KW and KH <= 3 and dil == 1 and (M % 4 or N % 4)):
        # channel counts off the split-fp16 kernel's 4-channel quads (the encoder's 81-channel input): zero-pad
        # to a multiple of 4, run the split-fp16 weight gradient and add the real channels' block into g
        def pad4(t):
            c = t.shape[3]
            if c % 4 == 0:
                return t
            tp = torch.zeros(t.shape[:3] + (c + (-c) % 4,), dtype=t.dtype, device=t.device)
            tp[..., :c] = t
            return tp
        gp = wgrad(pad4(a), pad4(x), KH, KW, dil, pad, circ, None, None)
        g += gp[:M, :N]
        return g
    p = WgradArgs()
    p.a, p.B, p.Ha, p.Wa, p.M = ptr(a), B, Ha, Wa, M
    p.x, p.Hx, p.Wx, p.N = ptr(x), Hx, Wx, N
    p.KH, p.KW, p.dil, p.pad_y, p.pad_x, p.circ = KH, KW, dil, pad[0], pad[1], circ
    p.g = ptr(g)
    if ops.CONV_PRECISION == ops.PREC_X3F16 and KH == KW and KH <= 3 and dil == 1 and M % 4 == 0 and N % 4 == 0:
        # operand ranges: the tensors' live range tags (written by the kernels that produced them), an absmax
        # pass only for a tensor without one (ops.input_tag); a_range: a's tag pointer when the caller has it
        ops.reserve_tags(a.device, 2)
        ar = a_range if a_range is not None else _range_ptr(a)
        xr = x_range if x_range is not None else _range_ptr(x)
        ws = torch.empty(lib.nps_wgrad_x3_ws_floats(M, N, KH, KW), dtype=torch.float32, device=a.device)
        p.db = ptr(db)  # (None -> NULL)
        arith = "x3w"

        fn = lib.nps_conv2d_wgrad_x3_set if store else lib.nps_conv2d_wgrad_x3

        def launch():
            check(fn(ctypes.byref(p), ar, xr, ptr(ws), stream_ptr()), "conv2d_wgrad_x3")
    else:
        arith = "f32w"

        def launch():
            check(lib.nps_conv2d_wgrad(ctypes.byref(p), stream_ptr()), "conv2d_wgrad")
    if ops.conv_probe is not None:  # bench.py's live roofline probe (ops.conv_probe)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        ops.conv_probe.append((e0, e1, 2.0 * B * Ha * Wa * M * N * KH * KW, (arith, KH * KW, 0),
                               4.0 * (a.numel() + x.numel() + g.numel())))
        if ops.conv_shape_log is not None:  # (tools/call_shapes.py --train)
            ops.conv_shape_log.append(dict(cin=N, cout=M, k=(KH, KW), hw=(Hx, Wx), out=(Ha, Wa), B=B, nsrc=1,
                                           acc=not store, addends=0, act=0, gn=False, pre_act=0, stats=False))
    else:
        launch()
    return g


def _range_ptr(t: torch.Tensor) -> int:
    """Device pointer of an upper bound of |t| (a range tag, include/nps.h): t's live tag, else a fresh absmax."""
    if ops.USE_IN_TAGS:
        return ops.input_tag(t)
    return ptr(_keep(ops.absmax(t)))


_KEEP = []


def _keep(t):
    """Hold a one-off range tensor (NPS_RANGE_TAGS without input tags) for the launches that read its pointer.
    The invariant that makes this safe: those launches are enqueued on the stream the tensor was allocated on
    (or on a side stream that is joined before the caller returns, before 8 more _keep calls can drop it), so the
    caching allocator's stream-ordered reuse cannot hand its memory out before they ran."""
    _KEEP.append(t)
    del _KEEP[:-8]
    return t


# the bias gradient of a conv from its weight-gradient launch (wgrad(db=...)) instead of a channel_sums pass over dy
# (dev knob NPS_FUSE_DB=0: off)
FUSE_DB = os.environ.get("NPS_FUSE_DB", "1") != "0"


def channel_sums(x: torch.Tensor) -> torch.Tensor:
    x = _c(x)
    C = x.shape[-1]
    out = torch.zeros(C, dtype=torch.float32, device=x.device)
    check(lib.nps_channel_sums(ptr(x), x.numel() // C, C, ptr(out), stream_ptr()), "channel_sums")
    return out


# Training forward convs carry the GroupNorm(1) moments of their outputs (nps_conv2d_t.out_stats), so the
# differentiable frames' group_norm_stats sums them instead of a statistics pass (dev knob NPS_CARRY_TRAIN=0: off)
CARRY_TRAIN = os.environ.get("NPS_CARRY_TRAIN", "1") != "0"


# the residual add of the differentiable path in one pass (nps_add_at_copy) instead of clone + nps_add_at
# (dev knob NPS_ADD_AT_COPY=0: off)
ADD_AT_COPY = os.environ.get("NPS_ADD_AT_COPY", "1") != "0"
# ... which also carries the sum's GroupNorm(1) moments (dev knob NPS_CARRY_ADD=0: off)
CARRY_ADD = os.environ.get("NPS_CARRY_ADD", "1") != "0"


def _carry_buffer(x):
    return ops.new_stats(x.shape[0], x) if CARRY_TRAIN and x.is_cuda and ops.CONV_PRECISION == ops.PREC_X3F16 else None


def _carry(y, st):
    if st is not None:
        ops.attach_stats(y, st)  # (ignored when the conv's kernel could not take the moments: incomplete)


def _pack_plain(w, dil=1):
    """Pack a [Cout][Cin][KH][KW] stride-1 conv weight (any derived tensor)."""
    return ops.pack_conv_weight(w, 1, dil)


# ------------------------------------------------------------------------- frame (cat/crop/GN/GELU)
class FrameFn(torch.autograd.Function):
    """act(GroupNorm(cat(crop_Nd(src_i)))) — proc_unet_modern.py:245-247, :191, :351; common.py:20-34."""

    @staticmethod
    def forward(ctx, meta, gamma, beta, *srcs):
        offsets, frame_hw, groups, eps, act = meta
        ss = [Src(_c(t), *o) for t, o in zip(srcs, offsets)]
        gn = None
        if gamma is not None:
            stats = ops.group_norm_stats(ss, frame_hw, groups)
            gn = ops.GN(stats, gamma.detach(), beta.detach(), groups, eps)
        out = ops.frame_pack(ss, frame_hw, gn, act)
        ctx.meta = meta
        ctx.has_gn = gamma is not None
        ctx.save_for_backward(*( [gamma, beta, gn.stats] if gn is not None else []), *[s.t for s in ss])
        return out

    @staticmethod
    def backward(ctx, gout):
        return _frame_bwd(ctx, gout, None)


# ResidualBlock's two uses of its input in one autograd node (frame_pair; dev knob NPS_FRAME_PAIR=0: two FrameFns)
FRAME_PAIR = os.environ.get("NPS_FRAME_PAIR", "1") != "0"


def _frame_bwd(ctx, gout, gplain):
    """FrameFn / FramePairFn backward: the sources' gradients (and GroupNorm affine's) in one frame-backward pass,
    gplain (the plain concatenation's gradient, or None) added inside it (nps_frame_pack_bwd2)."""
    offsets, frame_hw, groups, eps, act = ctx.meta
    saved = ctx.saved_tensors
    if ctx.has_gn:
        gamma, beta, stats = saved[:3]
        srcs = saved[3:]
    else:
        gamma = beta = stats = None
        srcs = saved
    gout = _c(gout)
    B = srcs[0].shape[0]
    Cin = sum(t.shape[3] for t in srcs)
    a = Conv2dArgs()
    a.nsrc = len(srcs)
    a.src = ops._c_src([Src(t, *o) for t, o in zip(srcs, offsets)])
    a.B, a.Hin, a.Win, a.Cin = B, frame_hw[0], frame_hw[1], Cin
    dgamma = dbeta = work = None
    if ctx.has_gn:
        a.gn_stats, a.gn_gamma, a.gn_beta = ptr(stats), ptr(gamma), ptr(beta)
        a.gn_groups, a.gn_eps = groups, eps
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
        work = ops.new_stats(B, gout, Cin)  # zero on entry (nps_frame_pack_bwd2): a slice of a zeroed chunk
    a.pre_act = act
    need = ctx.needs_input_grad[3:]
    dsrc = [torch.empty_like(t) if need[i] else None for i, t in enumerate(srcs)]
    arr = (ctypes.c_void_p * 3)(*[(d.data_ptr() if d is not None else None) for d in dsrc] +
                               [None] * (3 - len(dsrc)))
    # each source gradient leaves with a range tag: the conv backward reading it as dy needs no absmax pass
    tags = [None] * 3
    if ops.USE_OUT_TAGS:
        ops.reserve_tags(gout.device, len(dsrc))
        tags[:len(dsrc)] = [ops.new_tag(d) if d is not None else None for d in dsrc]
    tarr = (ctypes.c_void_p * 3)(*tags)
    gp = _c(gplain) if gplain is not None else None
    check(lib.nps_frame_pack_bwd2(ctypes.byref(a), ptr(gout), ptr(gp), arr, tarr, ptr(dgamma), ptr(dbeta),
                                  ptr(work), stream_ptr()), "frame_pack_bwd")
    return (None, dgamma, dbeta, *dsrc)


class FramePairFn(torch.autograd.Function):
    """(act(GroupNorm(cat(crop_Nd(src_i)))), cat(crop_Nd(src_i))) — a ResidualBlock's conv1 input and its shortcut's
    (or identity path's) input, proc_unet_modern.py:243-250 — from one node, so the backward adds the second
    output's gradient inside the frame backward (nps_frame_pack_bwd2) instead of autograd accumulating two
    gradients per source with a separate pass.  A single source covering the frame is returned as the plain
    output itself (a view: no copy)."""

    @staticmethod
    def forward(ctx, meta, gamma, beta, *srcs):
        offsets, frame_hw, groups, eps, act = meta
        ss = [Src(_c(t), *o) for t, o in zip(srcs, offsets)]
        gn = None
        if gamma is not None:
            stats = ops.group_norm_stats(ss, frame_hw, groups)
            gn = ops.GN(stats, gamma.detach(), beta.detach(), groups, eps)
        out = ops.frame_pack(ss, frame_hw, gn, act)
        ident = len(ss) == 1 and tuple(offsets[0]) == (0, 0) and tuple(srcs[0].shape[1:3]) == tuple(frame_hw)
        plain = srcs[0] if ident else ops.frame_pack(ss, frame_hw, None, 0)
        ctx.meta = meta
        ctx.has_gn = gamma is not None
        ctx.ident = ident
        ctx.save_for_backward(*([gamma, beta, gn.stats] if gn is not None else []), *[s.t for s in ss])
        return out, plain

    @staticmethod
    def backward(ctx, gout, gplain):
        if gout is None:  # (only the plain output was used)
            gout = torch.zeros((ctx.saved_tensors[-1].shape[0], *ctx.meta[1],
                                sum(t.shape[3] for t in ctx.saved_tensors[(3 if ctx.has_gn else 0):])),
                               dtype=torch.float32, device=gplain.device)
        return _frame_bwd(ctx, gout, gplain)


def frame_pair(srcs: Sequence[Src], frame_hw, norm=None, act=0):
    """(frame(srcs, norm, act), frame(srcs)) through FramePairFn: one frame backward for both consumers."""
    frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
    meta = (tuple((int(s.off_y), int(s.off_x)) for s in srcs), frame_hw,
            norm.num_groups if norm is not None else 0, float(norm.eps) if norm is not None else 0.0, act)
    gamma = norm.weight if norm is not None else None
    beta = norm.bias if norm is not None else None
    f, p = FramePairFn.apply(meta, gamma, beta, *[s.t for s in srcs])
    t0 = srcs[0].t
    if p._base is t0:  # the identity view carries the source's live range tag and moments (same version counter)
        for attr in ("_nps_tag", "_nps_stats"):
            if getattr(t0, attr, None) is not None:
                setattr(p, attr, getattr(t0, attr))
    return f, p


def frame(srcs: Sequence[Src], frame_hw, norm=None, act=0) -> torch.Tensor:
    """Materialise the virtual conv input frame (differentiably).  `norm` is an nn.GroupNorm or None."""
    frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
    if norm is None and act == 0 and len(srcs) == 1:
        s = srcs[0]
        if s.off_y == 0 and s.off_x == 0 and tuple(s.t.shape[1:3]) == frame_hw:
            return s.t
    meta = (tuple((int(s.off_y), int(s.off_x)) for s in srcs), frame_hw,
            norm.num_groups if norm is not None else 0, float(norm.eps) if norm is not None else 0.0, act)
    gamma = norm.weight if norm is not None else None
    beta = norm.bias if norm is not None else None
    return FrameFn.apply(meta, gamma, beta, *[s.t for s in srcs])


def crop(x: torch.Tensor, out_hw, off) -> torch.Tensor:
    """crop_Nd (common.py:20-34): place x at `off` inside a zero frame of size out_hw."""
    return frame([Src(x, off[0], off[1])], out_hw)


# ------------------------------------------------------------------------- conv
def _s2_phase_weight(w, ry, rx, p):
    """Input-gradient phase (ry, rx) of a stride-2 3x3 conv with top/left padding p in {0, 1}: dx[2q + r]
    sums dy[o] w[k] over 2o + k - p = 2q + r, i.e. o in {q - 1 + p, q + p}.  As a 2x2 conv of dy with top
    padding 1 - p, tap t reads dy[q - 1 + p + t] and uses kernel element k = r - p + 2 - 2t."""
    Cout, Cin, K, _ = w.shape
    out = torch.zeros((Cin, Cout, 2, 2), dtype=w.dtype, device=w.device)
    wt = w.detach().transpose(0, 1)
    for ty in range(2):
        ky = ry - p + 2 - 2 * ty
        if not 0 <= ky < K:
            continue
        for tx in range(2):
            kx = rx - p + 2 - 2 * tx
            if 0 <= kx < K:
                out[:, :, ty, tx] = wt[:, :, ky, kx]
    return out


class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d forward/backward (models/common.py:37-47): stride 1 (valid / zero / circular 'same',
    dilated) or the 3x3 stride-2 Downsample (proc_unet_modern.py:445-455, space-to-depth form)."""

    @staticmethod
    def forward(ctx, geo, x, weight, bias):
        KH, KW, s, d, lo, hi, circ = geo
        x = _c(x)
        B, H, W, Cin = x.shape
        Cout = weight.shape[0]
        if s == 2:
            if not (KH == 3 and KW == 3 and d == 1 and circ == 0 and lo == hi and lo[0] == lo[1] and lo[0] in (0, 1)):
                raise NotImplementedError("stride-2 conv: only the 3x3 U-Net Downsample form (padding 0 or 1)")
            p = lo[0]
            Ho, Wo = (H + 2 * p - 3) // 2 + 1, (W + 2 * p - 3) // 2 + 1
            xq = ops.space_to_depth(x, p, Ho + 1, Wo + 1)
            st = _carry_buffer(x)
            y = ops.conv2d([Src(xq)], (Ho + 1, Wo + 1), ops.cached_pack(weight, "s2d", ops.pack_conv_weight_s2d),
                           bias, Cout, 2, 2,
                           out_hw=(Ho, Wo), out_stats=st)
            _carry(y, st)
            ctx.save_for_backward(xq, weight)
        elif s == 1:
            wp = ops.cached_pack(weight, ("conv", 1, d), lambda w: ops.pack_conv_weight(w, 1, d))
            st = _carry_buffer(x)
            y = ops.conv2d([Src(x)], (H, W), wp, bias, Cout, KH, KW, dil=d, pad=lo,
                           pad_bottom=hi, circ=circ, out_stats=st)
            _carry(y, st)
            ctx.save_for_backward(x, weight)
        else:
            raise NotImplementedError(f"conv stride {s}")
        ctx.geo, ctx.in_hw, ctx.has_bias = geo, (H, W), bias is not None
        ctx.param = weight  # the nn.Parameter itself: its input-gradient packing is cached on it (ops.cached_pack)
        return y

    @staticmethod
    def backward(ctx, gy):
        KH, KW, s, d, lo, hi, circ = ctx.geo
        xs, w = ctx.saved_tensors
        gy = _c(gy)
        H, W = ctx.in_hw
        B, Ho, Wo, Cout = gy.shape
        Cin = w.shape[1]
        dx = dw = db = rng = None
        if ops.CONV_PRECISION == ops.PREC_X3F16 and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            # rng is a raw pointer into the tag arena, passed to every launch below: reserve the tags of the
            # WHOLE backward first (gy's tag; 2 per input-gradient conv — one, or four stride-2 phases; 2 for
            # the weight gradient), so no later reserve can wrap the arena (zeroing gy's tag) while rng is live
            ops.reserve_tags(gy.device, 1 + (2 if s == 1 else 8) + 2)
            rng = _range_ptr(gy)  # gradients: any magnitude (its tag, or one absmax pass shared by dx and dw)
        # the weight gradient reads only gy and x: it runs on a side stream beside the input-gradient conv(s)
        # (ops.Fork), each filling the CUs the other's last round leaves idle; joined before returning
        fork = ops.Fork(gy, on=ops.SIDE_WGRAD and ctx.needs_input_grad[1] and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1]:
            if s == 1:
                wd = ops.cached_pack(ctx.param, ("dgrad", d), lambda p: ops.pack_conv_weight_dgrad(p, d))
                if circ:
                    dx = ops.conv2d([Src(gy)], (Ho, Wo), wd, None, Cin, KH, KW, dil=d,
                                    circ=circ, out_hw=(H, W), in_scale=rng)
                else:
                    pt = (d * (KH - 1) - lo[0], d * (KW - 1) - lo[1])
                    dx = ops.conv2d([Src(gy)], (Ho, Wo), wd, None, Cin, KH, KW, dil=d,
                                    pad=pt, out_hw=(H, W), in_scale=rng)
            else:
                p = lo[0]
                dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=gy.device)
                for ry in range(2):
                    for rx in range(2):
                        hq, wq = (H - ry + 1) // 2, (W - rx + 1) // 2
                        if hq <= 0 or wq <= 0:
                            continue
                        ops.conv2d([Src(gy)], (Ho, Wo), _pack_plain(_s2_phase_weight(w, ry, rx, p)), None, Cin, 2, 2,
                                   pad=(1 - p, 1 - p), out_hw=(hq, wq), out=dx, out_os=2, out_off=(ry, rx),
                                   in_scale=rng)
        if ctx.needs_input_grad[2]:
            with fork:
                # the bias gradient from the weight-gradient launch's staging of gy (wgrad(db=...))
                db = (torch.empty(Cout, dtype=torch.float32, device=gy.device)
                      if ctx.has_bias and ctx.needs_input_grad[3] else None)
                if s == 1:
                    dw = wgrad(gy, xs, KH, KW, dil=d, pad=lo, circ=circ, a_range=rng, db=db)
                    if dw.shape[1] != Cin:      # input carried zero padding channels (packed encoder input)
                        dw = dw[:, :Cin].contiguous()
                else:
                    C = Cin
                    G = wgrad(gy, xs, 2, 2, a_range=rng, db=db)                # [Cout][4C][2][2]
                    G = G.view(Cout, 2, 2, C, 2, 2).permute(0, 3, 4, 1, 5, 2).reshape(Cout, C, 4, 4)
                    dw = G[:, :, :3, :3].contiguous()
            fork.join(dw, *([db] if db is not None else []))
        if ctx.has_bias and ctx.needs_input_grad[3] and db is None:
            db = channel_sums(gy)
        return None, dx, dw, db


class ConvTranspose2dFn(torch.autograd.Function):
    """nn.ConvTranspose2d(k=4, s=2) of the U-Net Upsample, optionally circularly pre-padded
    (ConvTranspose2d_padded, models/common.py:93-100; proc_unet_modern.py:425-436)."""

    @staticmethod
    def forward(ctx, geo, x, weight, bias):
        c, p = geo
        x = _c(x)
        B, H, W, Cin = x.shape
        Cout = weight.shape[1]
        Hp, Wp = H + 2 * c, W + 2 * c
        Ho, Wo = 2 * Hp + 2 - 2 * p, 2 * Wp + 2 - 2 * p
        out = ops.empty_nhwc(B, Ho, Wo, Cout, x)
        phases = ops.cached_pack(weight, "convT", ops.pack_convT_phases)
        st = _carry_buffer(x)  # (the 4 phases write disjoint elements: their moments add up to out's)
        for ph in range(4):
            py, px = ph >> 1, ph & 1
            ops.conv2d([Src(x)], (H, W), phases[ph], bias, Cout, 2, 2, pad=(1, 1), circ=c, out_hw=(Hp + 1, Wp + 1),
                       out=out, out_os=2, out_off=(py - p, px - p), out_stats=st)
        _carry(out, st)
        ctx.geo, ctx.has_bias = geo, bias is not None
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, gout):
        c, p = ctx.geo
        x, w = ctx.saved_tensors
        gout = _c(gout)
        B, H, W, Cin = x.shape
        Cout = w.shape[1]
        Hp, Wp = H + 2 * c, W + 2 * c
        # the transposed conv's adjoint is a 4x4 stride-2 conv of gout: space-to-depth + 2x2 conv
        dq = ops.space_to_depth(gout, p, Hp + 1, Wp + 1)                    # [B][Hp+1][Wp+1][4 Cout]
        dx = dw = db = None
        forked = ops.SIDE_WGRAD and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
        # dq is read by both streams: its range tag is settled before the fork point (ops.Fork settle)
        fork = ops.Fork(gout, on=forked, settle=[dq])
        if ctx.needs_input_grad[1]:
            w2 = w.detach().view(Cin, Cout, 2, 2, 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(Cin, 4 * Cout, 2, 2)
            dxp = ops.conv2d([Src(dq)], (Hp + 1, Wp + 1), _pack_plain(w2.contiguous()), None, Cin, 2, 2,
                             out_hw=(Hp, Wp))  # dq's range: its tag (ops.input_tag), shared from gout
            if c:
                dx = torch.empty_like(x)
                check(lib.nps_circular_fold(ptr(dxp), ptr(dx), B, H, W, Cin, c, stream_ptr()), "circular_fold")
            else:
                dx = dxp
        if ctx.needs_input_grad[2]:
            with fork:  # beside the input-gradient conv, as in Conv2dFn.backward
                if c:
                    xp = torch.empty((B, Hp, Wp, Cin), dtype=torch.float32, device=x.device)
                    check(lib.nps_circular_pad(ptr(x), ptr(xp), B, H, W, Cin, c, stream_ptr()), "circular_pad")
                else:
                    xp = x
                G = wgrad(xp, dq, 2, 2)                                            # [Cin][4 Cout][2][2]
                dw = G.view(Cin, 2, 2, Cout, 2, 2).permute(0, 3, 4, 1, 5, 2).reshape(Cin, Cout, 4, 4).contiguous()
            fork.join(dw)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = channel_sums(gout)
        return None, dx, dw, db


def conv2d(conv, x: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of a models.common.Conv2d on an NHWC tensor (no fused epilogue)."""
    return Conv2dFn.apply(conv.geometry(), x, conv.weight, conv.bias)


def conv_transpose2d(conv, x: torch.Tensor) -> torch.Tensor:
    if tuple(conv.kernel_size) != (4, 4) or tuple(conv.stride) != (2, 2) or tuple(conv.dilation) != (1, 1) \
            or tuple(conv.output_padding) != (0, 0) or conv.groups != 1 or conv.padding[0] != conv.padding[1] \
            or conv.padding[0] not in (0, 1):
        raise NotImplementedError("only the U-Net Upsample transposed conv (k=4, s=2) runs on the MI355X path")
    return ConvTranspose2dFn.apply((conv.pre_pad, conv.padding[0]), x, conv.weight, conv.bias)


# ------------------------------------------------------------------------- 3-D conv
def _check_geo3(geo):
    """The 3-D conv geometries that have a backward: K^3 in 1..3 at stride 1 — valid / zero-padded by at most K - 1,
    or circular 'same' — and the K = 3 stride-2 Downsample with zero padding 0 or 1."""
    K, s, circ, zpad = geo
    ok = 1 <= K <= 3 and circ >= 0 and zpad >= 0 and not (circ and zpad)
    if s == 1:
        ok = ok and zpad <= K - 1 and (circ == 0 or 2 * circ == K - 1)
    elif s == 2:
        if ok and circ:
            raise NotImplementedError("3-D stride-2 conv with circular padding has no backward on the MI355X path")
        ok = ok and K == 3 and zpad in (0, 1)
    else:
        ok = False
    if not ok:
        raise NotImplementedError(f"3-D conv backward: K={K} stride={s} circ={circ} zpad={zpad} is not supported")


def _fp32_3d(x, weight, what):
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise NotImplementedError(f"{what}: the 3-D convs differentiate fp32 tensors only (use fp32 for training)")
    if x.dim() != 5:
        raise RuntimeError(f"{what}: NDHWC input expected, got {tuple(x.shape)}")


def _pack3(w, transposed=False):
    return ops.pack_conv3d_weight(w, transposed=transposed)


class Conv3dFn(torch.autograd.Function):
    """nn.Conv3d forward/backward on NDHWC fp32 (models/common.py Conv3d.run3d): geo = Conv3d.geometry3d() =
    (K, stride, circ, zpad).  Input gradient = nps_conv3d_fwd launches on dy — stride 1: the conv with flipped,
    channel-swapped weights over dy extended by K - 1 - zpad zeros (circularly for circular 'same'); stride 2: one
    transposed-mode launch (8 K = 2 phases) with the k3 weight zero-padded to k4, shifted by -zpad and cropped to x,
    which stores every voxel of dx (those no output reads get exact zeros).  Weight gradient = nps_conv3d_wgrad."""

    @staticmethod
    def forward(ctx, geo, x, weight, bias):
        _check_geo3(geo)
        _fp32_3d(x, weight, "Conv3dFn")
        K, s, circ, zpad = geo
        x = _c(x)
        y = ops.conv3d([ops.Src3(x)], x.shape[1:4], ops.cached_pack(weight, "conv3", _pack3), bias, weight.shape[0], K,
                       stride=s, circ=circ, zpad=zpad)
        ctx.geo, ctx.has_bias = geo, bias is not None
        ctx.param = weight  # the nn.Parameter itself: its input-gradient packing is cached on it (ops.cached_pack)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        K, s, circ, zpad = ctx.geo
        x, w = ctx.saved_tensors
        gy = _c(gy)
        B, D, H, W, Cin = x.shape
        dx = dw = db = None
        fork = ops.Fork(gy, on=ops.SIDE_WGRAD and ctx.needs_input_grad[1] and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1]:
            if s == 1:
                wd = ops.cached_pack(ctx.param, "dgrad3", lambda p: _pack3(ops.conv3d_dgrad_weight(p)))
                dx = ops.conv3d([ops.Src3(gy)], gy.shape[1:4], wd, None, Cin, K, circ=circ,
                                zpad=0 if circ else K - 1 - zpad)
            else:
                wt = ops.cached_pack(ctx.param, "dgrad3_s2",
                                     lambda p: _pack3(ops.conv3d_s2_dgrad_weight(p), transposed=True))
                dx = torch.empty_like(x)
                ops.conv3d([ops.Src3(gy)], gy.shape[1:4], wt, None, Cin, 2, transposed=True, zpad=1, out=dx, out_os=2,
                           out_off=(-zpad,) * 3)
        if ctx.needs_input_grad[2]:
            with fork:  # beside the input-gradient conv, as in Conv2dFn.backward
                dw = ops.conv3d_wgrad(gy, x, K, stride=s, circ=circ, zpad=zpad)
            fork.join(dw)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = channel_sums(gy)
        return None, dx, dw, db


class ConvTranspose3dFn(torch.autograd.Function):
    """The 3-D U-Net Upsample on NDHWC fp32 (models/common.py ConvTranspose3d_padded): circular pad geo = (pad,),
    then nn.ConvTranspose3d(k=4, s=2, p=0).  The adjoint is the K = 4 / stride-2 conv of dy — a K = 2 conv over dy's
    space-to-depth form (8 Cout channels) — followed by the fold of the circular border onto the core; the weight
    gradient is the K = 4 / stride-2 nps_conv3d_wgrad with the roles swapped (a = the padded input, x = dy)."""

    @staticmethod
    def forward(ctx, geo, x, weight, bias):
        _fp32_3d(x, weight, "ConvTranspose3dFn")
        (c,) = geo
        x = _c(x)
        out = ops.conv3d([ops.Src3(x)], x.shape[1:4], ops.cached_pack(weight, "convT3", lambda p: _pack3(p, True)),
                         bias, weight.shape[1], 2, transposed=True, circ=c, zpad=1)
        ctx.geo, ctx.has_bias = geo, bias is not None
        ctx.param = weight
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, gout):
        (c,) = ctx.geo
        x, w = ctx.saved_tensors
        gout = _c(gout)
        B, D, H, W, Cin = x.shape
        Dp, Hp, Wp = D + 2 * c, H + 2 * c, W + 2 * c
        dx = dw = db = None
        fork = ops.Fork(gout, on=ops.SIDE_WGRAD and ctx.needs_input_grad[1] and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1]:
            dq = ops.space_to_depth3d(gout, Dp + 1, Hp + 1, Wp + 1)           # [B][Dp+1][Hp+1][Wp+1][8 Cout]
            wd = ops.cached_pack(ctx.param, "dgradT3", lambda p: _pack3(ops.conv_transpose3d_dgrad_weight(p)))
            dxp = ops.conv3d([ops.Src3(dq)], dq.shape[1:4], wd, None, Cin, 2)
            dx = ops.circular_fold3d(dxp, c) if c else dxp
        if ctx.needs_input_grad[2]:
            with fork:
                dw = ops.conv3d_wgrad(ops.circular_pad3d(x, c) if c else x, gout, 4, stride=2)
            fork.join(dw)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = channel_sums(gout)
        return None, dx, dw, db


def conv3d(conv, x: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of a models.common.Conv3d on an NDHWC fp32 tensor."""
    return Conv3dFn.apply(conv.geometry3d(), x, conv.weight, conv.bias)


def conv_transpose3d(conv, x: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of a models.common.ConvTranspose3d_padded on an NDHWC fp32 tensor."""
    if (set(conv.kernel_size) != {4} or set(conv.stride) != {2} or set(conv.padding) != {0}
            or set(conv.output_padding) != {0} or set(conv.dilation) != {1} or conv.groups != 1):
        raise NotImplementedError("3-D Upsample: ConvTranspose3d(k=4, s=2, p=0) only")
    return ConvTranspose3dFn.apply((conv.pad,), x, conv.weight, conv.bias)


# ------------------------------------------------------------------------- 1-D conv (k taps along L)
def _check_geo1(geo):
    """The 1-D conv geometries that run: K in 1..4 at stride 1 zero-padded by at most K - 1 per side, or stride 2."""
    K, s, pl, pr = geo
    ok = 1 <= K <= 4 and s in (1, 2) and pl >= 0 and pr >= 0 and (s == 2 or (pl <= K - 1 and pr <= K - 1))
    if not ok:
        raise NotImplementedError(f"1-D conv: K={K} stride={s} padding=({pl}, {pr}) is not supported")


def _fp32_1d(x, weight, what):
    if not (x.is_cuda and weight.is_cuda):
        raise RuntimeError(f"nps_hip ops run on the MI355X only: {what} got a tensor on {x.device} / {weight.device}")
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise NotImplementedError(f"{what}: the 1-D convs run fp32 tensors only")
    if x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError(f"{what}: a (B, 1, L, C) input expected, got {tuple(x.shape)}")


def _rows(x):
    """(B, 1, L, C) -> the contiguous (B, L, C) view."""
    x = _c(x)
    return x.view(x.shape[0], x.shape[2], x.shape[3])


def _map(y):
    """(B, L, C) -> (B, 1, L, C)."""
    return y.view(y.shape[0], 1, y.shape[1], y.shape[2])


def _pack1_phases(w):
    return [ops.pack_conv1d_weight(p) for p in ops.conv_transpose1d_phase_weights(w)]


def _conv_transpose1d_fwd(x3, phases, bias, Cout, p):
    """The k4/s2 transposed conv (padding p) of x3 (B, L, Cin) as its two 2-tap phases, written interleaved."""
    B, L, _ = x3.shape
    out = torch.empty((B, 2 * L + 2 - 2 * p, Cout), dtype=torch.float32, device=x3.device)
    for r in (0, 1):  # q in [0, L]: positions -p .. 2 L + 1 - p, every element of out once
        ops.conv1d([ops.Src1(x3)], L, phases[r], bias, Cout, 2, pad=(1, 1), out=out, out_os=2, out_off=r - p)
    return out


class Conv1dFn(torch.autograd.Function):
    """nn.Conv1d forward/backward on (B, 1, L, C) fp32 maps (models/common.py Conv1d.run_ad): geo = (K, stride,
    pad_left, pad_right), zero padding.  Input gradient = nps_conv1d_fwd launches on dy — stride 1: the conv with
    flipped, channel-swapped taps padded by K - 1 - pad; stride 2: the two 2-tap phases (out_os = 2) of the
    transposed conv whose weight is the conv's own, shifted by -pad_left and cropped to x.  Weight gradient =
    nps_conv1d_wgrad, bias gradient = channel_sums."""

    @staticmethod
    def forward(ctx, geo, x, weight, bias):
        _check_geo1(geo)
        _fp32_1d(x, weight, "Conv1dFn")
        K, s, pl, pr = geo
        x3 = _rows(x)
        y = ops.conv1d([ops.Src1(x3)], x3.shape[1], ops.cached_pack(weight, "conv1", ops.pack_conv1d_weight), bias,
                       weight.shape[0], K, stride=s, pad=(pl, pr))
        ctx.geo, ctx.has_bias = geo, bias is not None
        ctx.param = weight  # the nn.Parameter itself: its input-gradient packings are cached on it
        ctx.save_for_backward(x3, weight)
        return _map(y)

    @staticmethod
    def backward(ctx, gy):
        K, s, pl, pr = ctx.geo
        x3, w = ctx.saved_tensors
        gy = _rows(gy)
        B, L, Cin = x3.shape
        Ly = gy.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            if s == 1:
                wd = ops.cached_pack(ctx.param, "dgrad1",
                                     lambda p: ops.pack_conv1d_weight(ops.conv1d_dgrad_weight(p)))
                dx = ops.conv1d([ops.Src1(gy)], Ly, wd, None, Cin, K, pad=(K - 1 - pl, K - 1 - pr))
            else:
                # dx[i] = sum over 2 o + t - pl = i of dy[o] w[:, :, t]: the stride-2 transposed conv of dy with the
                # conv's own weight as (in = Cout, out = Cin, k); positions 2 q + r - pl, q in [0, Ly]
                ph = ops.cached_pack(ctx.param, "dgrad1_s2", _pack1_phases)
                covered = 2 * Ly + 1 - pl >= L - 1
                dx = (torch.empty if covered else torch.zeros)((B, L, Cin), dtype=torch.float32, device=gy.device)
                for r in (0, 1):
                    ops.conv1d([ops.Src1(gy)], Ly, ph[r], None, Cin, 2, pad=(1, 1), out=dx, out_os=2, out_off=r - pl)
            dx = _map(dx)
        if ctx.needs_input_grad[2]:
            dw = ops.conv1d_wgrad(gy, x3, K, stride=s, pad=(pl, pr))
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = channel_sums(gy)
        return None, dx, dw, db


class ConvTranspose1dFn(torch.autograd.Function):
    """nn.ConvTranspose1d(k=4, s=2, padding p in {0, 1}) on (B, 1, L, C) fp32 maps: the two 2-tap phases of
    nps_conv1d_fwd.  The input gradient is the K = 4 / stride-2 / pad-p conv of dy with the parameter read as
    (out = Cin, in = Cout, k); the weight gradient is nps_conv1d_wgrad with the roles swapped (a = x, x = dy)."""

    @staticmethod
    def forward(ctx, p, x, weight, bias):
        _fp32_1d(x, weight, "ConvTranspose1dFn")
        x3 = _rows(x)
        out = _conv_transpose1d_fwd(x3, ops.cached_pack(weight, "convT1", _pack1_phases), bias, weight.shape[1], p)
        ctx.p, ctx.has_bias = p, bias is not None
        ctx.param = weight
        ctx.save_for_backward(x3, weight)
        return _map(out)

    @staticmethod
    def backward(ctx, gout):
        p = ctx.p
        x3, w = ctx.saved_tensors
        gout = _rows(gout)
        Cin = x3.shape[2]
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            wd = ops.cached_pack(ctx.param, "dgradT1", ops.pack_conv1d_weight)
            dx = _map(ops.conv1d([ops.Src1(gout)], gout.shape[1], wd, None, Cin, 4, stride=2, pad=(p, p)))
        if ctx.needs_input_grad[2]:
            dw = ops.conv1d_wgrad(x3, gout, 4, stride=2, pad=(p, p))
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = channel_sums(gout)
        return None, dx, dw, db


def check_conv_transpose1d(conv):
    if (tuple(conv.kernel_size) != (4,) or tuple(conv.stride) != (2,) or conv.padding[0] not in (0, 1)
            or tuple(conv.output_padding) != (0,) or tuple(conv.dilation) != (1,) or conv.groups != 1):
        raise NotImplementedError("1-D Upsample: ConvTranspose1d(k=4, s=2, padding 0 or 1) only on the MI355X path")


def conv1d(conv, x: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of a zero-padded k-tap models.common.Conv1d on a (B, 1, L, C) fp32 map."""
    return Conv1dFn.apply(conv.geometry1d(), x, conv.weight, conv.bias)


def conv_transpose1d(conv, x: torch.Tensor) -> torch.Tensor:
    """Differentiable forward of a models.common.ConvTranspose1d on a (B, 1, L, C) fp32 map."""
    check_conv_transpose1d(conv)
    return ConvTranspose1dFn.apply(conv.padding[0], x, conv.weight, conv.bias)


# ------------------------------------------------------------------------- 3-D frame (cat/crop/GN/GELU)
def _frame3d_fwd(meta, gamma, beta, srcs):
    """The forward shared by Frame3dFn / FramePair3dFn: (Src3 sources, GN or None, act(GN(frame)))."""
    offsets, frame_dhw, groups, eps, act = meta
    for t in srcs:
        if t.dtype != torch.float32 or t.dim() != 5:
            raise NotImplementedError(f"3-D frame: fp32 NDHWC sources only (use fp32 for training), got {t.dtype} "
                                      f"{tuple(t.shape)}")
    ss = [ops.Src3(_c(t), *o) for t, o in zip(srcs, offsets)]
    gn = None
    if gamma is not None:  # a pass over the frame (carried moments stay with the inference path)
        gn = ops.GN(ops.gn_stats3d(ss, frame_dhw, groups), gamma.detach(), beta.detach(), groups, eps)
    return ss, gn, ops.frame3d(ss, frame_dhw, gn, act)


def _frame3d_save(ctx, meta, gamma, beta, gn, ss):
    ctx.meta = meta
    ctx.has_gn = gn is not None
    ctx.save_for_backward(*([gamma, beta, gn.stats] if gn is not None else []), *[s.t for s in ss])


def _frame3d_bwd(ctx, gout, gplain):
    """Frame3dFn / FramePair3dFn backward: the sources' gradients (and the GroupNorm affine's) in one
    nps_frame3d_bwd, gplain (the plain concatenation's gradient, or None) added inside it."""
    offsets, frame_dhw, groups, eps, act = ctx.meta
    saved = ctx.saved_tensors
    gn = None
    if ctx.has_gn:
        gamma, beta, stats = saved[:3]
        gn = ops.GN(stats, gamma, beta, groups, eps)
        saved = saved[3:]
    ss = [ops.Src3(t, *o) for t, o in zip(saved, offsets)]
    dsrc, dgamma, dbeta = ops.frame3d_bwd(ss, frame_dhw, gn, act, _c(gout), _c(gplain) if gplain is not None else None,
                                          ctx.needs_input_grad[3:])
    return (None, dgamma, dbeta, *dsrc)


class Frame3dFn(torch.autograd.Function):
    """act(GroupNorm(cat(crop_Nd(src_i)))) on NDHWC fp32 — FrameFn in 3-D (proc_unet_modern.py:245-247, :191 with
    num_spatial_dims=3): offsets along D, H and W, exactly Cin channels."""

    @staticmethod
    def forward(ctx, meta, gamma, beta, *srcs):
        ss, gn, out = _frame3d_fwd(meta, gamma, beta, srcs)
        _frame3d_save(ctx, meta, gamma, beta, gn, ss)
        return out

    @staticmethod
    def backward(ctx, gout):
        return _frame3d_bwd(ctx, gout, None)


class FramePair3dFn(torch.autograd.Function):
    """(act(GroupNorm(cat(crop_Nd(src_i)))), cat(crop_Nd(src_i))) from one node — FramePairFn in 3-D: a ResidualBlock's
    conv1 input and its shortcut's (or identity path's) input, so the backward adds the second output's gradient
    inside the frame backward.  A single source covering the frame is returned as the plain output itself (a view)."""

    @staticmethod
    def forward(ctx, meta, gamma, beta, *srcs):
        offsets, frame_dhw = meta[0], meta[1]
        ss, gn, out = _frame3d_fwd(meta, gamma, beta, srcs)
        ident = len(ss) == 1 and not any(offsets[0]) and tuple(srcs[0].shape[1:4]) == tuple(frame_dhw)
        plain = srcs[0] if ident else ops.frame3d(ss, frame_dhw)
        _frame3d_save(ctx, meta, gamma, beta, gn, ss)
        return out, plain

    @staticmethod
    def backward(ctx, gout, gplain):
        if gout is None:  # (only the plain output was used)
            srcs = ctx.saved_tensors[(3 if ctx.has_gn else 0):]
            gout = torch.zeros((srcs[0].shape[0], *ctx.meta[1], sum(t.shape[4] for t in srcs)), dtype=torch.float32,
                               device=gplain.device)
        return _frame3d_bwd(ctx, gout, gplain)


def _frame3d_meta(srcs, frame_dhw, norm, act):
    return (tuple((int(s.off_d), int(s.off_h), int(s.off_w)) for s in srcs), tuple(int(v) for v in frame_dhw),
            norm.num_groups if norm is not None else 0, float(norm.eps) if norm is not None else 0.0, act)


def frame_pair3d(srcs: Sequence[ops.Src3], frame_dhw, norm=None, act=0):
    """(frame3d(srcs, norm, act), frame3d(srcs)) through FramePair3dFn: one frame backward for both consumers."""
    return FramePair3dFn.apply(_frame3d_meta(srcs, frame_dhw, norm, act), norm.weight if norm is not None else None,
                               norm.bias if norm is not None else None, *[s.t for s in srcs])


def frame3d(srcs: Sequence[ops.Src3], frame_dhw, norm=None, act=0) -> torch.Tensor:
    """Materialise the virtual NDHWC conv input frame (differentiably).  `norm` is an nn.GroupNorm or None."""
    meta = _frame3d_meta(srcs, frame_dhw, norm, act)
    if norm is None and act == 0 and len(srcs) == 1 and not any(meta[0][0]) \
            and tuple(srcs[0].t.shape[1:4]) == meta[1]:
        return srcs[0].t
    return Frame3dFn.apply(meta, norm.weight if norm is not None else None, norm.bias if norm is not None else None,
                           *[s.t for s in srcs])


def crop3d(x: torch.Tensor, out_dhw, off) -> torch.Tensor:
    """crop_Nd (common.py:20-34) in 3-D: place x at `off` inside a zero frame of size out_dhw."""
    return frame3d([ops.Src3(x, *off)], out_dhw)


class AddAt3dFn(torch.autograd.Function):
    """base + crop_Nd(src) placed at `off` on NDHWC fp32 (the residual `crop_Nd(h) + shortcut`,
    proc_unet_modern.py:250 in 3-D; off = (0, 0, 0) and equal sizes is a plain sum, proc_ufno.py:118)."""

    @staticmethod
    def forward(ctx, off, base, src):
        ctx.off, ctx.src_dhw = off, tuple(src.shape[1:4])
        return ops.add_at_copy3d(_c(base), _c(src), off)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        gs = None
        if ctx.needs_input_grad[2]:  # the adjoint of the placement: crop_Nd of g at the negated offsets
            gs = ops.frame3d([ops.Src3(g, *(-o for o in ctx.off))], ctx.src_dhw)
        return None, g, gs


def add_at3d(base, src, off=(0, 0, 0)):
    return AddAt3dFn.apply(tuple(int(o) for o in off), base, src)


# ------------------------------------------------------------------------- element-wise
class GeluFn(torch.autograd.Function):
    """nn.GELU() (erf form)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        y = torch.empty_like(x)
        check(lib.nps_gelu(ptr(x), ptr(y), x.numel(), stream_ptr()), "gelu")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = _c(gy)
        gx = torch.empty_like(x)
        check(lib.nps_gelu_bwd(ptr(x), ptr(gy), ptr(gx), x.numel(), stream_ptr()), "gelu_bwd")
        return gx


def gelu(x):
    return GeluFn.apply(x)


def act(x, code):
    return gelu(x) if code == GELU else x


class AddAtFn(torch.autograd.Function):
    """base + crop_Nd(src) placed at `off` (the residual `crop_Nd(h) + shortcut`, proc_unet_modern.py:250;
    off = (0, 0) and equal sizes is a plain sum, e.g. proc_ufno.py:118, proc_dilatedresnet.py:49)."""

    @staticmethod
    def forward(ctx, off, base, src):
        base, src = _c(base), _c(src)
        B, Ho, Wo, C = base.shape
        Hs, Ws = src.shape[1:3]
        if C % 4 == 0 and ADD_AT_COPY:  # one pass: out = base + crop_Nd(src) (nps_add_at_copy)
            out = torch.empty_like(base)
            st = _carry_buffer(base) if CARRY_ADD else None  # out's GroupNorm(1) moments, for the next frame
            check(lib.nps_add_at_copy(ptr(out), ptr(base), ptr(src), B, Ho, Wo, Hs, Ws, C, off[0], off[1], ptr(st),
                                      stream_ptr()), "add_at_copy")
            _carry(out, st)
        else:
            out = base.clone()
            check(lib.nps_add_at(ptr(out), ptr(src), B, Ho, Wo, Hs, Ws, C, off[0], off[1], stream_ptr()), "add_at")
        ctx.off, ctx.src_hw = off, (Hs, Ws)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        gs = None
        if ctx.needs_input_grad[2]:
            gs = ops.frame_pack([Src(g, -ctx.off[0], -ctx.off[1])], ctx.src_hw)
        return None, g, gs


def add_at(base, src, off=(0, 0)):
    return AddAtFn.apply((int(off[0]), int(off[1])), base, src)


class NchwToNhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.nchw_to_nhwc(x)

    @staticmethod
    def backward(ctx, g):
        return ops.nhwc_to_nchw(_c(g))


class NhwcToNchwFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.nhwc_to_nchw(_c(x))

    @staticmethod
    def backward(ctx, g):
        return ops.nchw_to_nhwc(_c(g))


def to_nhwc(x):
    return NchwToNhwcFn.apply(x)


def to_nchw(x):
    return NhwcToNchwFn.apply(x)


# ------------------------------------------------------------------------- spectral conv
# One Function per dimension.  meta[0] is the activation layout, ops.NhwcW or ops.NchwW (ops.py, W-pass adapters): it
# issues the W passes, and everything between them is written once, here and in ops.spectral2d_fwd / spectral3d_fwd.
def _spec2d_bwd_mid(ctx, gZ):
    """The layout-independent middle of the SpectralConv2d backward: gZ (the W pass's adjoint of gy) ->
    (gX2, gwp, dp, dWf, dbf).  With FiLM the unscaled mixer output is formed again from the saved X2 (never Y / S)."""
    _, m1, m2, Cout, mode = ctx.meta
    B, H, W, Cin = ctx.shape
    X2, wpack, *film = ctx.saved_tensors
    R = X2.shape[1]
    dev = gZ.device
    s = stream_ptr()
    c64 = torch.complex64
    gY = torch.empty((B, R, m2, Cout), dtype=c64, device=dev)
    gX2 = torch.empty((B, R, m2, Cin), dtype=c64, device=dev)
    gwp = torch.empty((R, m2, Cin, Cout), dtype=c64, device=dev)
    check(lib.nps_spectral_dft_h(ptr(gZ), ptr(gY), B, H, m1, m2, Cout, s), "spectral_dft_h (bwd)")
    dp = dWf = dbf = None
    if film:
        S, p, Wf = film
        Yu = torch.empty((B, R, m2, Cout), dtype=c64, device=dev)
        gS = torch.empty((B, R, m2, Cout), dtype=torch.float32, device=dev)
        check(lib.nps_spectral_mix(ptr(X2), ptr(wpack), ptr(Yu), B, R, m2, Cin, Cout, s), "spectral_mix (bwd)")
        check(lib.nps_spectral_film_bwd(ptr(Yu), ptr(S), ptr(gY), ptr(gS), B, R, m2, Cout, s), "spectral_film_bwd")
        need = ctx.needs_input_grad[5:8]
        dp = torch.empty_like(p) if need[0] else None
        dWf = torch.empty_like(Wf) if need[1] else None
        dbf = torch.empty((Wf.shape[0],), dtype=torch.float32, device=dev) if need[2] else None
        if any(need):
            check(lib.nps_spectral_film_param_bwd(ptr(gS), ptr(p), ptr(Wf), ptr(dWf), ptr(dbf), ptr(dp), B, p.shape[1],
                                                  Cout, H, m1, m2, mode, s), "spectral_film_param_bwd")
    check(lib.nps_spectral_mix_bwd(ptr(X2), ptr(wpack), ptr(gY), ptr(gX2), ptr(gwp), B, R, m2, Cin, Cout, s),
          "spectral_mix_bwd")
    return gX2, gwp, dp, dWf, dbf


class SpectralConv2dFn(torch.autograd.Function):
    """SpectralConv2d.forward (proc_fno.py:257-288) and its torch.fft / complex-einsum backward, on NHWC x
    (B, H, W, Cin) or, with no transposes, on the module's own NCHW x (B, Cin, H, W) (meta's layout).  With FiLM
    conditioning (:271-284; p, Wf, bf given, else None) the mixed modes are multiplied by the real factor S
    (ops.film_scale) of p (B, K) and weights_feat, which then get gradients too.  Saved: (X2, wpack[, S, p, Wf])."""

    @staticmethod
    def forward(ctx, meta, x, w1, w2, wpack, p, Wf, bf):
        Lay, m1, m2, Cout, mode = meta
        lay = Lay.of(x)
        film = None if p is None else (_c(p), _c(Wf), _c(bf), mode)
        X2, Z, S = ops.spectral2d_fwd(lay, wpack, m1, m2, Cout, film=film)
        y = lay.new_out(Cout)
        lay.idft_w(Z, y, m2, Cout)
        ctx.meta, ctx.shape = meta, lay.dims
        ctx.save_for_backward(X2, wpack, *(() if film is None else (S, film[0], film[1])))
        return y

    @staticmethod
    def backward(ctx, gy):
        Lay, m1, m2, Cout, _ = ctx.meta
        B, H, W, Cin = ctx.shape
        dev = gy.device
        s = stream_ptr()
        gZ = torch.empty((B, H, m2, Cout), dtype=torch.complex64, device=dev)
        Lay.idft_w_bwd(gy, gZ, B, H, W, m2, Cout)
        gX2, gwp, dp, dWf, dbf = _spec2d_bwd_mid(ctx, gZ)
        dx = dw1 = dw2 = None
        if ctx.needs_input_grad[1]:
            gX1 = torch.empty((B, H, m2, Cin), dtype=torch.complex64, device=dev)
            check(lib.nps_spectral_idft_h(ptr(gX2), ptr(gX1), B, H, m1, m2, Cin, s), "spectral_idft_h (bwd)")
            dx = Lay.dft_w_bwd(gX1, B, H, W, m2, Cin)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw1 = torch.empty((Cin, Cout, m1, m2), dtype=torch.complex64, device=dev)
            dw2 = torch.empty((Cin, Cout, m1, m2), dtype=torch.complex64, device=dev)
            check(lib.nps_spectral_unpack_grad(ptr(gwp), ptr(dw1), ptr(dw2), Cin, Cout, H, m1, m2, s),
                  "spectral_unpack_grad")
        return None, dx, dw1, dw2, None, dp, dWf, dbf


def _spectral_conv2d(Lay, module, x, H, p=None):
    mode, Wf, bf = (None, None, None) if p is None else (int(module.transform_mode), module.weights_feat.weight,
                                                         module.weights_feat.bias)
    return SpectralConv2dFn.apply((Lay, module.modes1, module.modes2, module.out_channels, mode), x, module.weights1,
                                  module.weights2, module.packed(H), p, Wf, bf)


def spectral_conv2d(module, x):
    return _spectral_conv2d(ops.NhwcW, module, x, x.shape[1])


def spectral_conv2d_nchw(module, x):
    return _spectral_conv2d(ops.NchwW, module, x, x.shape[2])


def spectral_conv2d_film(module, x, p):
    assert p is not None  # proc_fno.py:272: we must have supplied params
    return _spectral_conv2d(ops.NhwcW, module, x, x.shape[1], p)


def spectral_conv2d_film_nchw(module, x, p):
    assert p is not None  # proc_fno.py:272: we must have supplied params
    return _spectral_conv2d(ops.NchwW, module, x, x.shape[2], p)


class SpectralConv3dFn(torch.autograd.Function):
    """SpectralConv3d.forward (proc_fno.py:334-376) and its torch.fft / complex-einsum backward, axis by axis with
    the 2-D kernels (include/nps.h, SpectralConv3d), on the NDHWC view x (B, D*H, W, Cin) or, with no transposes, on
    the module's own NCDHW x (B, Cin, D, H, W) (meta's layout).  Saved: (X3, wpack)."""

    @staticmethod
    def forward(ctx, meta, x, w1, w2, w3, w4, wpack):
        Lay, m1, m2, m3, Cout, D = meta
        lay = Lay.of(x)
        B, DH, W, Cin = lay.dims
        y = lay.new_out(Cout)
        X3 = ops.spectral3d_fwd(lay, D, wpack, m1, m2, m3, Cout, y)
        ctx.meta, ctx.shape, ctx.xshape = meta, (B, D, DH // D, W, Cin), tuple(x.shape)
        ctx.save_for_backward(X3, wpack)
        return y

    @staticmethod
    def backward(ctx, gy):
        Lay, m1, m2, m3, Cout, _ = ctx.meta
        B, D, H, W, Cin = ctx.shape
        X3, wpack = ctx.saved_tensors
        R1, R2 = min(D, 2 * m1), min(H, 2 * m2)
        dev = gy.device
        c64 = torch.complex64
        s = stream_ptr()
        gZ2 = torch.empty((B, D * H, m3, Cout), dtype=c64, device=dev)
        gZ1 = torch.empty((B * D, R2, m3, Cout), dtype=c64, device=dev)
        gY = torch.empty((B, R1, R2 * m3, Cout), dtype=c64, device=dev)
        gX3 = torch.empty((B, R1, R2 * m3, Cin), dtype=c64, device=dev)
        gwp = torch.empty((R1, R2, m3, Cin, Cout), dtype=c64, device=dev)
        Lay.idft_w_bwd(gy, gZ2, B, D * H, W, m3, Cout)
        check(lib.nps_spectral_dft_h(ptr(gZ2), ptr(gZ1), B * D, H, m2, m3, Cout, s), "spectral3d dft_h (H, bwd)")
        check(lib.nps_spectral_dft_h(ptr(gZ1), ptr(gY), B, D, m1, R2 * m3, Cout, s), "spectral3d dft_h (D, bwd)")
        check(lib.nps_spectral_mix_bwd(ptr(X3), ptr(wpack), ptr(gY), ptr(gX3), ptr(gwp), B, R1, R2 * m3, Cin, Cout,
                                       s), "spectral3d mix_bwd")
        dx = None
        gws = [None] * 4
        if ctx.needs_input_grad[1]:
            gX2 = torch.empty((B, D, R2 * m3, Cin), dtype=c64, device=dev)
            gX1 = torch.empty((B * D, H, m3, Cin), dtype=c64, device=dev)
            check(lib.nps_spectral_idft_h(ptr(gX3), ptr(gX2), B, D, m1, R2 * m3, Cin, s), "spectral3d idft_h (D, bwd)")
            check(lib.nps_spectral_idft_h(ptr(gX2), ptr(gX1), B * D, H, m2, m3, Cin, s), "spectral3d idft_h (H, bwd)")
            dx = Lay.dft_w_bwd(gX1, B, D * H, W, m3, Cin).view(ctx.xshape)
        if any(ctx.needs_input_grad[2:6]):
            gws = [torch.empty((Cin, Cout, m1, m2, m3), dtype=c64, device=dev) for _ in range(4)]
            check(lib.nps_spectral3d_unpack_grad(ptr(gwp), *[ptr(g) for g in gws], Cin, Cout, D, H, m1, m2, m3, s),
                  "spectral3d_unpack_grad")
        return (None, dx, *gws, None)


def _spectral_conv3d(Lay, module, x, D, H):
    return SpectralConv3dFn.apply((Lay, module.modes1, module.modes2, module.modes3, module.out_channels, D), x,
                                  module.weights1, module.weights2, module.weights3, module.weights4,
                                  module.packed(D, H))


def spectral_conv3d(module, x, D):
    """x: (B, D*H, W, Cin) NDHWC view -> (B, D*H, W, Cout)."""
    return _spectral_conv3d(ops.NhwcW, module, x, D, x.shape[1] // D)


def spectral_conv3d_nchw(module, x):
    """x: (B, Cin, D, H, W) -> (B, Cout, D, H, W)."""
    return _spectral_conv3d(ops.NchwW, module, x, x.shape[2], x.shape[3])


# ------------------------------------------------------------------------- spectral conv, 1-D
class SpectralConv1dFn(torch.autograd.Function):
    """SpectralConv1d.forward (proc_fno.py:199-222) on channels-last x (B, L, Cin) (or its (B, 1, L, Cin) view) and
    its torch.fft / complex-einsum backward (SURVEY.md §0.8 in one dimension).  With FiLM conditioning (:209-218; p,
    Wf, bf given, else None) the mixed modes are multiplied by the real factor S (ops.film1d_scale), and p and
    weights_feat's weight and bias get gradients too.  Saved: (X, wpack[, S, p, Wf])."""

    @staticmethod
    def forward(ctx, meta, x, w, wpack, p, Wf, bf):
        m, Cout, mode = meta
        x = _c(x)
        B, L, Cin = x.shape[0], x.shape[-2], x.shape[-1]
        film = None if p is None else (_c(p), _c(Wf), _c(bf), mode)
        X, Y, S = ops.spectral1d_mid([Src(x)], wpack, m, Cout, film=film)
        y = ops.spectral1d_idft(Y, L).reshape(x.shape[:-1] + (Cout,))
        ctx.meta, ctx.shape, ctx.xshape = meta, (B, L, Cin), tuple(x.shape)
        ctx.save_for_backward(X, wpack, *(() if film is None else (S, film[0], film[1])))
        return y

    @staticmethod
    def backward(ctx, gy):
        m, Cout, mode = ctx.meta
        B, L, Cin = ctx.shape
        X, wpack, *film = ctx.saved_tensors
        gy = _c(gy)
        dev = gy.device
        s = stream_ptr()
        c64 = torch.complex64
        gY = ops.spectral1d_dft([Src(gy.reshape(B, L, Cout))], m, adjoint=True)  # irfft's adjoint: c_k / L
        dp = dWf = dbf = None
        if film:
            S, p, Wf = film
            # the unscaled mixer output again from the saved X (never Y / S: S may be zero)
            Yu = torch.empty((B, m, Cout), dtype=c64, device=dev)
            gS = torch.empty((B, m, Cout), dtype=torch.float32, device=dev)
            check(lib.nps_spectral_mix(ptr(X), ptr(wpack), ptr(Yu), B, 1, m, Cin, Cout, s), "spectral_mix (bwd)")
            check(lib.nps_spectral_film_bwd(ptr(Yu), ptr(S), ptr(gY), ptr(gS), B, 1, m, Cout, s), "spectral_film_bwd")
            need = ctx.needs_input_grad[4:7]
            dp = torch.empty_like(p) if need[0] else None
            dWf = torch.empty_like(Wf) if need[1] else None
            dbf = torch.empty((Wf.shape[0],), dtype=torch.float32, device=dev) if need[2] else None
            if any(need):
                check(lib.nps_spectral1d_film_param_bwd(ptr(gS), ptr(p), ptr(Wf), ptr(dWf), ptr(dbf), ptr(dp), B,
                                                        p.shape[1], Cout, m, mode, s), "spectral1d_film_param_bwd")
        gX = torch.empty((B, m, Cin), dtype=c64, device=dev)
        gwp = torch.empty((lib.nps_spectral1d_mix_bwd_parts(B), m, Cin, Cout), dtype=c64, device=dev)  # result: part 0
        check(lib.nps_spectral1d_mix_bwd(ptr(X), ptr(wpack), ptr(gY), ptr(gX), ptr(gwp), B, m, Cin, Cout, s),
              "spectral1d_mix_bwd")
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dx = ops.spectral1d_idft(gX, L, adjoint=True).reshape(ctx.xshape)
        if ctx.needs_input_grad[2]:
            dw = torch.empty((Cin, Cout, m), dtype=c64, device=dev)
            check(lib.nps_spectral1d_unpack_grad(ptr(gwp), ptr(dw), Cin, Cout, m, s), "spectral1d_unpack_grad")
        return None, dx, dw, None, dp, dWf, dbf


def spectral_conv1d(module, x):
    return SpectralConv1dFn.apply((module.modes1, module.out_channels, None), x, module.weights1, module.packed(),
                                  None, None, None)


def spectral_conv1d_film(module, x, p):
    assert p is not None  # proc_fno.py:210: we must have supplied params
    return SpectralConv1dFn.apply((module.modes1, module.out_channels, int(module.transform_mode)), x,
                                  module.weights1, module.packed(), p, module.weights_feat.weight,
                                  module.weights_feat.bias)


# ------------------------------------------------------------------------- decoder / wrapper / loss
class TimeConvDecodeFn(torch.autograd.Function):
    """TimeConvDense conv1d chain + add_delta('per_step') + tanh + spatial-cond mask
    (dec_grid.py:126-146, :8-31; activation_wrapper.py:34-35)."""

    @staticmethod
    def forward(ctx, meta, pre, u, w1, b1, w2, b2, dtcum, mask):
        mask_ch, act_tanh, num_c, tw = meta
        pre, u = _c(pre), _c(u)
        out = ops.timeconv_decode(pre, u, w1.detach().contiguous(), b1.detach(), w2.detach().contiguous(),
                                  b2.detach(), dtcum, mask, mask_ch, act_tanh, num_c, tw)
        ctx.meta = meta
        ctx.save_for_backward(pre, u, w1, b1, w2, b2, dtcum, mask if mask is not None else torch.empty(0))
        ctx.has_mask = mask is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        mask_ch, act_tanh, num_c, tw = ctx.meta
        pre, u, w1, b1, w2, b2, dtcum, mask = ctx.saved_tensors
        mask = mask if ctx.has_mask else None
        gout = _c(gout)
        B, H, W = u.shape[0], 1, ops.grid_pixels(u)  # per pixel: a grid of any dimension as its flat pixels
        ka, kb = w1.shape[2], w2.shape[2]
        C2 = 2 * num_c
        nparams = C2 * num_c * ka + C2 + num_c * C2 * kb + num_c
        nblk = B * ((H * W + 63) // 64)
        ws = torch.empty((nblk, nparams), dtype=torch.float32, device=gout.device)
        gpre = torch.empty_like(pre)
        S = 0 if mask is None else mask.shape[1]
        check(lib.nps_timeconv_decode_bwd(ptr(pre), ptr(u), ptr(w1.detach().contiguous()), ptr(b1.detach()),
                                          ptr(w2.detach().contiguous()), ptr(b2.detach()), ptr(dtcum), ptr(mask), S,
                                          mask_ch, ptr(gout), ptr(gpre), ptr(ws), B, num_c, tw, H, W,
                                          1 if act_tanh else 0, stream_ptr()), "timeconv_decode_bwd")
        red = channel_sums(ws)
        o = 0
        gw1 = red[o:o + C2 * num_c * ka].view_as(w1)
        o += C2 * num_c * ka
        gb1 = red[o:o + C2]
        o += C2
        gw2 = red[o:o + num_c * C2 * kb].view_as(w2)
        o += num_c * C2 * kb
        gb2 = red[o:o + num_c]
        return None, gpre, None, gw1, gb1, gw2, gb2, None, None


class DecodeChainFn(torch.autograd.Function):
    """ops.decode_chain (the per-pixel Conv1d chain of the grid decoders + add_delta + tanh + mask) and its HIP
    backward nps_decode_bwd: gradients of x (in x's layout) and of the stages' weights and biases; u is data."""

    @staticmethod
    def forward(ctx, spec, x, u, w1, b1, w2, b2, dtcum, mask):
        x, u = _c(x), _c(u)
        ws = [None if w is None else w.detach().contiguous() for w in (w1, b1, w2, b2)]
        out = ops.decode_chain(spec, x, u, *ws, dtcum, mask)
        ctx.spec = spec
        ctx.present = [t is not None for t in (w1, b1, w2, b2, dtcum, mask)]
        ctx.save_for_backward(x, u, *[t for t in (w1, b1, w2, b2, dtcum, mask) if t is not None])
        return out

    @staticmethod
    def backward(ctx, gout):
        x, u = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        w1, b1, w2, b2, dtcum, mask = [rest.pop(0) if have else None for have in ctx.present]
        ws = [None if w is None else w.detach().contiguous() for w in (w1, b1, w2, b2)]
        gout = _c(gout)
        d = ops.decode_args(ctx.spec, x, u, *ws, dtcum, mask)
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[1] else None
        gp = [torch.empty_like(w) if (w is not None and need[3 + i]) else None for i, w in enumerate(ws)]
        work = None
        if any(g is not None for g in gp):
            work = torch.empty(lib.nps_decode_bwd_ws_floats(ctypes.byref(d)), dtype=torch.float32, device=x.device)
        check(lib.nps_decode_bwd(ctypes.byref(d), ptr(gout), ptr(gx), ptr(gp[0]), ptr(gp[1]), ptr(gp[2]), ptr(gp[3]),
                                 ptr(work), stream_ptr()), "decode_chain_bwd")
        return None, gx, None, gp[0], gp[1], gp[2], gp[3], None, None


class VolumeRescaleFn(torch.autograd.Function):
    """activation_wrapper 'individual_static' volume preservation + re-applied mask
    (activation_wrapper.py:80-105); x (the model input) is data and gets no gradient."""

    @staticmethod
    def forward(ctx, meta, u, x, mpdcum, mask):
        mask_ch = meta
        u = _c(u)
        B, c, tw, H, W = u.shape
        xc = _c(x)
        new_tot = ops.plane_sums(u, 0, H * W, H * W, B * c * tw)
        prev_tot = ops.plane_sums(xc, (xc.shape[2] - 1) * H * W, xc.shape[2] * H * W, H * W, B * c)
        out = u.clone()
        ops.volume_rescale(out, new_tot, prev_tot, mpdcum, mask, mask_ch)
        ctx.meta = meta
        ctx.has_mask = mask is not None
        ctx.save_for_backward(u, new_tot, prev_tot, mpdcum, mask if mask is not None else torch.empty(0))
        return out

    @staticmethod
    def backward(ctx, g):
        mask_ch = ctx.meta
        u, new_tot, prev_tot, mpdcum, mask = ctx.saved_tensors
        mask = mask if ctx.has_mask else None
        g = _c(g)
        B, c, tw, H, W = u.shape
        S = 0 if mask is None else mask.shape[1]
        D = torch.empty(B * c * tw, dtype=torch.float64, device=g.device)
        check(lib.nps_plane_dot(ptr(g), ptr(u), ptr(mask), S, mask_ch, B, c * tw, H, W, ptr(D), stream_ptr()),
              "plane_dot")
        gu = torch.empty_like(u)
        check(lib.nps_volume_rescale_bwd(ptr(g), ptr(new_tot), ptr(prev_tot), ptr(mpdcum), ptr(mask), S, mask_ch,
                                         ptr(D), ptr(gu), B, c, tw, H, W, stream_ptr()), "volume_rescale_bwd")
        return None, gu, None, None, None


class VolumeModeFn(torch.autograd.Function):
    """activation_wrapper 'block' / 'individual' volume preservation + re-applied mask (activation_wrapper.py:40-79);
    meta = (mask_ch, mode, max_pct_dif).  x (the model input) is data and gets no gradient."""

    @staticmethod
    def forward(ctx, meta, u, x, mask):
        mask_ch, mode, m = meta
        u = _c(u)
        B, c, tw, H, W = u.shape
        xc = _c(x)
        new_tot = ops.plane_sums(u, 0, H * W, H * W, B * c * tw)
        prev_tot = ops.plane_sums(xc, (xc.shape[2] - 1) * H * W, xc.shape[2] * H * W, H * W, B * c)
        F = ops.volume_factors(new_tot, prev_tot, mode, m, B, c, tw)
        out = ops.volume_apply(u.clone(), F, mask, mask_ch)
        ctx.meta = meta
        ctx.has_mask = mask is not None
        ctx.save_for_backward(u, new_tot, prev_tot, F, mask if mask is not None else torch.empty(0))
        return out

    @staticmethod
    def backward(ctx, g):
        mask_ch, mode, m = ctx.meta
        u, new_tot, prev_tot, F, mask = ctx.saved_tensors
        mask = mask if ctx.has_mask else None
        g = _c(g)
        B, c, tw, H, W = u.shape
        S = 0 if mask is None else mask.shape[1]
        D = torch.empty(B * c * tw, dtype=torch.float64, device=g.device)
        check(lib.nps_plane_dot(ptr(g), ptr(u), ptr(mask), S, mask_ch, B, c * tw, H, W, ptr(D), stream_ptr()),
              "plane_dot")
        ws = torch.empty_like(D) if mode == "individual" else None  # p_i of the recomputed recurrence
        coef = torch.empty_like(F)
        check(lib.nps_volume_factors_bwd(ptr(new_tot), ptr(prev_tot), ptr(D), ops.VOLUME_MODES[mode], float(m),
                                         ptr(ws), ptr(coef), B, c, tw, stream_ptr()), "volume_factors_bwd")
        gu = torch.empty_like(u)
        check(lib.nps_volume_apply_bwd(ptr(g), ptr(F), ptr(coef), ptr(mask), S, mask_ch, ptr(gu), B, c, tw, H, W,
                                       stream_ptr()), "volume_apply_bwd")
        return None, gu, None, None


class SqrtMseSumFn(torch.autograd.Function):
    """torch.sqrt(nn.MSELoss(reduction='sum')(pred, labels)) — autoregressivepushforwardtrainer.py:158-162."""

    @staticmethod
    def forward(ctx, pred, labels):
        pred, labels = _c(pred), _c(labels)
        L = ops.sq_err_sum(pred, labels)        # fp64 on device
        r = torch.sqrt(L)
        ctx.save_for_backward(pred, labels, r)
        return r.float()

    @staticmethod
    def backward(ctx, g):
        pred, labels, r = ctx.saved_tensors
        scale = (g.double() / r).reshape(1)      # d sqrt(L) / d pred = (pred - labels) / sqrt(L)
        out = torch.empty_like(pred)
        check(lib.nps_scaled_diff(ptr(pred), ptr(labels), ptr(scale), ptr(out), pred.numel(), stream_ptr()),
              "scaled_diff")
        return out, None


def sqrt_mse_sum(pred, labels):
    return SqrtMseSumFn.apply(pred, labels)


class MseSumFn(torch.autograd.Function):
    """nn.MSELoss(reduction='sum')(pred, labels) as an fp64 device scalar with a HIP backward — a rank's
    part S_r of the global sum under data parallelism (trainers.distributed.global_sqrt_loss)."""

    @staticmethod
    def forward(ctx, pred, labels):
        pred, labels = _c(pred), _c(labels)
        ctx.save_for_backward(pred, labels)
        return ops.sq_err_sum(pred, labels)     # fp64

    @staticmethod
    def backward(ctx, g):
        pred, labels = ctx.saved_tensors
        scale = (2.0 * g.double()).reshape(1)     # d S / d pred = 2 (pred - labels)
        out = torch.empty_like(pred)
        check(lib.nps_scaled_diff(ptr(pred), ptr(labels), ptr(scale), ptr(out), pred.numel(), stream_ptr()),
              "scaled_diff")
        return out, None


def mse_sum(pred, labels):
    return MseSumFn.apply(pred, labels)


# ------------------------------------------------------------------------- U-Net self-attention
class AttentionFn(torch.autograd.Function):
    """proc_unet_modern.py:300-308 (column softmax) on qkv (B, N, heads * 3 * dk); saves qkv and the column
    log-sum-exp, and the backward recomputes the weights from them (nps_attn_bwd)."""

    @staticmethod
    def forward(ctx, meta, qkv):
        heads, dk, scale = meta
        qkv = _c(qkv)
        out, lse = ops.attention(qkv, heads, dk, scale)
        ctx.meta = meta
        ctx.save_for_backward(qkv, lse)
        return out

    @staticmethod
    def backward(ctx, gout):
        heads, dk, scale = ctx.meta
        qkv, lse = ctx.saved_tensors
        return None, ops.attention_bwd(qkv, lse, _c(gout), heads, dk, scale)


def attention(qkv: torch.Tensor, heads: int, dk: int, scale: float) -> torch.Tensor:
    return AttentionFn.apply((int(heads), int(dk), float(scale)), qkv)
