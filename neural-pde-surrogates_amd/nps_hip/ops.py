"""Torch-tensor front end of the HIP kernels (include/nps.h).

Activations are NHWC fp32 tensors of shape (B, H, W, C).  A conv input is a
*virtual frame*: a list of `Src(tensor, off_y, off_x)` slices concatenated
along channels, each placed at an offset of the frame (crop_Nd, cat), so no
cat / pad / crop is ever materialised.
"""
import ctypes
import math
import os
import weakref
from typing import List, NamedTuple, Optional, Sequence, Union

import torch

from . import Conv1dArgs, Conv2dArgs, Conv3dArgs, DecodeArgs, PackJob, Wgrad1dArgs, Wgrad3dArgs, Src as _CSrc, Src3 as _CSrc3, check, lib, ptr, stream_ptr

GELU = 1

# Conv arithmetic (include/nps.h NPS_PREC_*): exact fp32 MFMA, or the 3-pass split-fp16 MFMA products
# (~2^-21 relative per product, 5.3x the fp32 MFMA rate) for the stride-1 undilated 1x1 / 2x2 / 3x3 convs.
PREC_F32, PREC_X3F16 = 0, 1
# split-fp16 3x3 convs apply their GroupNorm / GELU prologue while staging (nps_conv2d_x3_prologue_ok)
# instead of a frame_pack pass in front of the conv (dev knob NPS_FUSE_PROLOGUE=0: off).  Pays off on the
# wide 192-channel tiles, whose producers stage each patch once for all output channels.
FUSE_PROLOGUE = os.environ.get("NPS_FUSE_PROLOGUE", "1") == "1"
# dev knob NPS_FUSE_PROLOGUE_1X1=0: the 1x1 convs' GroupNorm + GELU prologue materialised by frame_pack (A/B of the
# LDS-weight kernel's fused prologue, conv1x1_wl_kernel<6, 2, true>)
FUSE_PROLOGUE_1X1 = os.environ.get("NPS_FUSE_PROLOGUE_1X1", "1") != "0"
CONV_PRECISION = PREC_F32 if os.environ.get("NPS_CONV_PRECISION", "x3f16") == "f32" else PREC_X3F16
# the Downsample's 2x2 conv reads the space-to-depth view of its input directly (nps_conv2d_t.s2d) instead of
# a space_to_depth copy (dev knob NPS_S2D_VIEW=0: the copy)
S2D_VIEW = os.environ.get("NPS_S2D_VIEW", "1") == "1"
# split-fp16 transposed convs run their 4 phases in one launch (dev knob NPS_CONVT_MERGE=0: 4 launches)
MERGE_CONVT_PHASES = os.environ.get("NPS_CONVT_MERGE", "1") == "1"


def conv_precision(KH, KW, stride=1, dil=1):
    """Arithmetic a conv of this geometry runs in under the current CONV_PRECISION setting."""
    if CONV_PRECISION == PREC_X3F16 and lib.nps_conv2d_x3_eligible(KH, KW, stride, dil):
        return PREC_X3F16
    return PREC_F32

# Optional live probe of the conv kernel (bench.py): when a list, every conv2d launch appends
# (start_event, end_event, algorithmic_flops) recorded on the launching stream.
conv_probe = None
conv_shape_log = None  # dev (tools/call_shapes.py): with conv_probe, one launch-geometry dict per conv launch


class Src(NamedTuple):
    t: torch.Tensor          # (B, H, W, C) NHWC contiguous
    off_y: int = 0
    off_x: int = 0


# ----------------------------------------------------------------- range tags ----
# A split-fp16 conv scales its input by a power of 2 picked from an upper bound of |x| (include/nps.h,
# nps_conv2d_t.in_scale / in_tag*), so fp32-class accuracy holds for activations of any magnitude.  The
# bound travels with the tensor as a RANGE TAG: NPS_TAG_FLOATS floats of a per-device arena, raised by
# the kernel that writes the tensor (conv / frame_pack / spectral epilogues: out_tag).  A tensor without
# a live tag (model inputs, views, torch-made tensors) gets one from nps_absmax the first time a
# split-fp16 conv reads it.  Tags are only ever raised, so a tag shared by several tensors (a clone,
# a space-to-depth copy) or written by several kernels (accumulating convs) stays an upper bound.
TAG_FLOATS = 64 * 64        # NPS_TAG_FLOATS
# dev knob NPS_RANGE_TAGS: "1" (default) input + output tags, "in" / "out" one side only, "0" none
_TAGS = os.environ.get("NPS_RANGE_TAGS", "1")
USE_IN_TAGS, USE_OUT_TAGS = _TAGS in ("1", "in"), _TAGS in ("1", "out")
_ARENA_TAGS = 2048          # 32 MiB per device; re-zeroed (new generation) when exhausted


class _TagArena:
    def __init__(self, device):
        self.buf = torch.zeros(_ARENA_TAGS * TAG_FLOATS, dtype=torch.float32, device=device)
        self.gen = 0
        self.next = 0

    def reserve(self, k: int):
        """Start a new generation now unless k more tags fit in this one: a launch that needs several
        tags reserves them all before it reads any tag pointer, so no wrap (which zeroes the buffer)
        can happen between reading an input tag and launching the kernel that reads it."""
        if self.next + k > _ARENA_TAGS:
            # stream-ordered after every kernel that used the old generation; once side streams (Fork) have
            # carried launches, the device drains before and after the zero so no stream's kernel can read
            # or raise a tag across it (a wrap comes every few model calls)
            fenced = _forked and self.buf.is_cuda
            if fenced:
                torch.cuda.synchronize(self.buf.device)
            self.buf.zero_()
            if fenced:
                torch.cuda.synchronize(self.buf.device)
            self.gen += 1
            self.next = 0

    def alloc(self):
        self.reserve(1)
        i = self.next
        self.next += 1
        return _Tag(self, self.gen, self.buf.data_ptr() + 4 * i * TAG_FLOATS)


class _Tag(NamedTuple):
    arena: "_TagArena"
    gen: int
    ptr: int

    @property
    def live(self):
        return self.arena.gen == self.gen


_arenas = {}
_forked = False  # set by the first Fork that runs launches on a side stream


# ----------------------------------------------------------------- side streams ----
# Launches that do not depend on the one just issued (the ResidualBlock's 1x1 shortcut beside conv1, the U-FNO
# block's FNO layer beside its U-Net) go to a second HIP stream, so their work-groups take the CUs a
# persistent 3x3 launch leaves idle in its last round (B = 2: the 258^2 convs are 1122 tiles on 256 CUs,
# 4.4 rounds).  Each lane is one stream per device (one hardware queue).  dev knob NPS_SIDE_STREAM=0: off.
SIDE_STREAM = os.environ.get("NPS_SIDE_STREAM", "1") == "1"
SIDE_FNO = os.environ.get("NPS_SIDE_FNO", "1") == "1"      # dev knob: the U-FNO block's FNO layer fork
# ... for 2-D activations of at most this many elements (B=2 C3: 25 M; at B=16, 201 M, the U-Net's launches
# keep the CUs busy: within noise, profiles/r4/experiments/side_stream_*; the 3-D U-FNO forks at every size)
SIDE_FNO_MAX_ELEMS = int(float(os.environ.get("NPS_SIDE_FNO_MAX_ELEMS", "6.4e7")))


# dev knob NPS_SIDE_WGRAD=1: the training backward's weight gradients on a side stream (see
# nps_hip.autograd.Conv2dFn.backward)
SIDE_WGRAD = os.environ.get("NPS_SIDE_WGRAD", "0") == "1"


def fno_fork(h: torch.Tensor, settle: Sequence[torch.Tensor] = ()) -> "Fork":
    """The U-FNO block's fork for its FNO layer (lane 1): on for small activations (see SIDE_FNO_MAX_ELEMS)."""
    return Fork(h, lane=1, on=SIDE_FNO and h.numel() <= SIDE_FNO_MAX_ELEMS, settle=settle)
# dev knob: the shortcut fork needs conv1's last round to leave at least this fraction of the CUs idle
SIDE_MIN_IDLE = float(os.environ.get("NPS_SIDE_MIN_IDLE", "0.25"))
_side_streams = {}
_side_depth = 0   # > 0 while launches go to a side stream


_ncu = {}


def x3_plan_tiles(Ho: int, Wo: int, B: int, Cout: int, Cin: int, K: int = 3) -> int:
    """Work-group tiles of a stride-1 split-fp16 KxK launch with that output, as nps_conv2d_plan tiles it
    (wide 192-channel or 64-channel tiles, the planner's TH x TW): host-only, cached per shape."""
    key = (Ho, Wo, B, Cout, Cin, K)
    n = _plan_tiles.get(key)
    if n is None:
        a = Conv2dArgs()
        a.nsrc = 1
        a.src[0].ptr, a.src[0].C, a.src[0].H, a.src[0].W = 0x1000, Cin, Ho + K - 1, Wo + K - 1
        a.B, a.Hin, a.Win, a.Cin = B, Ho + K - 1, Wo + K - 1, Cin
        a.KH = a.KW = K
        a.stride, a.dil = 1, 1
        a.Hout, a.Wout, a.Cout = Ho, Wo, Cout
        a.out_C, a.out_H, a.out_W, a.out_os = Cout, Ho, Wo, 1
        a.precision = PREC_X3F16
        if lib.nps_conv2d_plan(ctypes_byref(a)) < 0:
            raise RuntimeError("conv2d_plan failed: " + lib.nps_last_error().decode())
        nco = 192 if a.TH * a.TW == 128 else 64
        n = _plan_tiles[key] = -(-Ho // a.TH) * -(-Wo // a.TW) * B * -(-Cout // nco)
    return n


_plan_tiles = {}


def last_round_idle(Ho: int, Wo: int, B: int, Cout: int, device, Cin: int = 192) -> float:
    """Fraction of the CUs left idle in the last round of a split-fp16 3x3 launch: the persistent grid of
    nps_launch_conv2d_x3 (one work-group per CU, multi_processor_count & ~7 of them) over the tiles
    nps_conv2d_plan picks (x3_plan_tiles).  A fork beside such a launch pays only when this is large: every
    cross-stream wait costs ~15 us (profiles/r4/experiments/side_stream_forks_ab.txt)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    n = _ncu.get(idx)
    if n is None:
        n = _ncu[idx] = torch.cuda.get_device_properties(idx).multi_processor_count & ~7
    return idle_fraction(x3_plan_tiles(Ho, Wo, B, Cout, Cin), n)


def idle_fraction(tiles: int, workgroups: int) -> float:
    """Idle share of a persistent grid of `workgroups` in the last round of `tiles` tiles."""
    last = tiles % workgroups
    return 0.0 if last == 0 else 1.0 - last / workgroups


class Fork:
    """`f = Fork(t)` marks the fork point on the current stream (t: any tensor of the device);
    `with f:` issues the enclosed launches on side stream `lane`, which starts at the fork point;
    `f.join(*outs)` makes the current stream wait for them and hands it the tensors they allocated.
    Moments buffers made inside (new_stats) are private zeros of the side stream; the tag arena fences a
    wrap across all streams.  `settle`: fp32 tensors both streams may read as split-fp16 conv inputs — their
    range tags are made live here, before the fork point, because a tag one stream computes lazily (absmax)
    could be read by the other before that absmax ran.  A no-op on the CPU or with NPS_SIDE_STREAM=0."""

    def __init__(self, like: torch.Tensor, lane: int = 0, on: bool = True, settle: Sequence[torch.Tensor] = ()):
        d = like.device
        self.on = on and SIDE_STREAM and d.type == "cuda"
        self.done = None
        if not self.on:
            return
        if USE_IN_TAGS and CONV_PRECISION == PREC_X3F16:
            ts = [t for t in settle if t is not None and t.dtype == torch.float32]
            reserve_tags(d, len(ts))
            for t in ts:
                input_tag(t)
        idx = d.index if d.index is not None else torch.cuda.current_device()
        key = (idx, lane)
        self.side = _side_streams.get(key)
        if self.side is None:
            self.side = _side_streams[key] = torch.cuda.Stream(device=idx)
        self.main = torch.cuda.current_stream(idx)
        self.start = torch.cuda.Event()
        self.start.record(self.main)

    def __enter__(self):
        global _side_depth, _forked
        if self.on:
            _forked = True
            self.side.wait_event(self.start)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
            _side_depth += 1
        return self

    def __exit__(self, *exc):
        global _side_depth
        if self.on:
            _side_depth -= 1
            self._ctx.__exit__(*exc)
            self.done = torch.cuda.Event()
            self.done.record(self.side)
        return False

    def join(self, *outs):
        if self.done is not None:
            self.main.wait_event(self.done)
            for t in outs:
                if isinstance(t, torch.Tensor):
                    t.record_stream(self.main)
            self.done = None


def _arena(device) -> _TagArena:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ar = _arenas.get(key)
    if ar is None:
        ar = _arenas[key] = _TagArena(device)
    return ar


def reserve_tags(device, k: int):
    """Guarantee that the next k tag allocations on `device` do not wrap the arena (see _TagArena.reserve)."""
    _arena(device).reserve(k)


def tag_of(t: torch.Tensor):
    """The live range tag of `t`, or None.  A tag is recorded with the tensor's version counter: a torch
    in-place write (add_, mul_, slice assignment) bumps t._version and so invalidates the bound; the HIP
    kernels that write into an existing tensor raise its tag instead."""
    rec = getattr(t, "_nps_tag", None)
    if rec is None:
        return None
    tag, ver = rec
    return tag if (tag.live and ver == t._version) else None


def _attach_tag(t: torch.Tensor, tag):
    t._nps_tag = (tag, t._version)


def new_tag(t: torch.Tensor) -> int:
    """Attach a fresh (zero) tag to `t`, whose writer will raise it; returns its device pointer."""
    tag = _arena(t.device).alloc()
    _attach_tag(t, tag)
    return tag.ptr


def out_tag(t: torch.Tensor, accumulate: bool) -> int:
    """Tag pointer for a kernel that writes into the existing tensor `t`: its live tag, or a new one —
    seeded with max|t| when the kernel accumulates onto (reads) the current contents.  Otherwise the
    contents the kernel leaves unwritten must be zeros or absent (crop padding, phase outputs)."""
    tag = tag_of(t)
    if tag is not None:
        return tag.ptr
    p = new_tag(t)
    if accumulate:
        check(lib.nps_absmax_into(ptr(t), t.numel(), p, stream_ptr()), "absmax (tag seed)")  # (fresh: zero)
    return p


def share_tag(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst holds a subset of src's values (and zeros): it may carry src's bound."""
    tag = tag_of(src)
    if tag is not None:
        _attach_tag(dst, tag)
    return dst


def input_tag(t: torch.Tensor) -> int:
    """Tag pointer bounding |t| for a split-fp16 conv reading t (nps_absmax when t has no live tag).

    On a side stream (inside a Fork) the fresh tag is PRIVATE, not attached to t: t may be an input both
    streams read (its settled tag died in an arena wrap inside the fork), and a tag attached here would be
    raised by an absmax queued only on the side stream, which a later main-stream launch reading t could
    see before that absmax ran.  The main stream measures t itself."""
    tag = tag_of(t)
    if tag is not None:
        return tag.ptr
    p = _arena(t.device).alloc().ptr if _side_depth > 0 else new_tag(t)
    check(lib.nps_absmax_into(ptr(t), t.numel(), p, stream_ptr()), "absmax (input tag)")  # (fresh arena tag: zero)
    return p


# ------------------------------------------------------------ GroupNorm(1) moments ----
# A split-fp16 2x2/3x3 conv that writes a whole tensor can add the per-sample (sum, sum of squares) of
# the values it stores to a zeroed fp64 [B][2] buffer (nps_conv2d_t.out_stats).  The tensor then CARRIES
# its moments (attach_stats), and the GroupNorm(1) of a frame made of such tensors (ResidualBlock.norm1 /
# norm2, proc_unet_modern.py:235-236) is their sum — no statistics pass over the frame.  Sources without
# moments get them from one nps_group_norm_stats pass over that source alone, kept for later frames.
# Moments are valid while the tensor is unchanged: torch's in-place ops bump t._version, and the HIP ops
# that write into an existing tensor drop them (drop_stats).
STATS_SUB = lib.nps_stats_sub()  # NPS_STATS_SUB of the loaded library (sub-slots of a moments buffer)


_STATS_CHUNK = 1 << 15      # doubles zeroed at once; slices are handed out and never re-zeroed
_stats_chunks = {}


def new_stats(B: int, like: torch.Tensor, sub: int = STATS_SUB) -> torch.Tensor:
    """A zeroed fp64 [B][sub][2] moments buffer: sub = NPS_STATS_SUB for nps_conv2d_t.out_stats, 1 for the
    [B][G][2] statistics a GroupNorm prologue reads (G = 1).  Slices of one zero-filled chunk per device
    (one fill launch per chunk instead of one per buffer); a chunk is never reused in place — it is freed
    when its last slice is."""
    n = B * sub * 2
    d = like.device
    key = (d.type, d.index if d.index is not None else torch.cuda.current_device())
    ch = _stats_chunks.get(key)
    if n > _STATS_CHUNK // 4 or _side_depth > 0:  # (a side stream's buffers are zeroed on that stream)
        return torch.zeros((B, sub, 2), dtype=torch.float64, device=d)
    if ch is None or ch[1] + n > _STATS_CHUNK:
        ch = [torch.zeros(_STATS_CHUNK, dtype=torch.float64, device=d), 0]
        _stats_chunks[key] = ch
    v = ch[0][ch[1]:ch[1] + n].view(B, sub, 2)
    ch[1] += (n + 31) // 32 * 32
    return v


def _stats_sum(parts, B, out):
    """out[b][0] = sum of the parts' (sum, sum of squares) over their sub-slots (nps_stats_sum)."""
    p = list(parts) + [None] * (3 - len(parts))
    n = [t.shape[1] if t is not None else 0 for t in p]
    check(lib.nps_stats_sum(ptr(p[0]), n[0], ptr(p[1]), n[1], ptr(p[2]), n[2], B, ptr(out), out.shape[1],
                            stream_ptr()), "stats_sum")
    return out


def attach_stats(t: torch.Tensor, st: torch.Tensor) -> torch.Tensor:
    """Record that st holds t's GroupNorm(1) moments (every element of t was added exactly once)."""
    if not getattr(st, "_nps_incomplete", False):
        t._nps_stats = (st, t._version)
    return t


def pixel_view(t: torch.Tensor, shape) -> torch.Tensor:
    """t.view(shape) of a channels-last tensor whose pixels are only arranged differently ((B, D*H, W, C) <->
    (B, D, H, W, C), (B, 1, L, C) <-> (B, L/32, 32, C)): the view keeps t's range tag and its GroupNorm(1) moments,
    which are a bound on, and sums over, the same elements."""
    v = share_tag(t.view(shape), t)
    st = stats_of(t)
    return attach_stats(v, st) if st is not None else v


def drop_stats(t: torch.Tensor):
    if getattr(t, "_nps_stats", None) is not None:
        t._nps_stats = None


_DEBUG_STATS = os.environ.get("NPS_DEBUG_STATS") == "1"  # dev: print every GroupNorm statistics pass and its caller


def stats_of(t: torch.Tensor) -> Optional[torch.Tensor]:
    """t's live GroupNorm(1) moments, or None."""
    rec = getattr(t, "_nps_stats", None)
    if rec is None:
        return None
    st, ver = rec
    return st if ver == t._version else None


def source_stats(t: torch.Tensor) -> torch.Tensor:
    """t's GroupNorm(1) moments: carried, or one nps_group_norm_stats pass (then carried).  Read-only:
    seed a buffer of your own with copy_stats() to accumulate into."""
    st = stats_of(t)
    if st is None:
        if _DEBUG_STATS:
            import traceback
            print("nps stats pass (source)", tuple(t.shape), "".join(traceback.format_stack(limit=5)[:-1]), flush=True)
        st = new_stats(t.shape[0], t, 1)
        check(lib.nps_group_norm_stats(_c_src([Src(t)]), 1, t.shape[0], t.shape[1], t.shape[2], t.shape[3], 1,
                                       ptr(st), 0, stream_ptr()), "group_norm_stats (source)")
        attach_stats(t, st)
    return st


def copy_stats(st: torch.Tensor) -> torch.Tensor:
    """A new out_stats buffer seeded with st's moments (to accumulate a conv's changes into)."""
    return _stats_sum([st], st.shape[0], new_stats(st.shape[0], st))


def _c_src(srcs: Sequence[Src]):
    arr = (_CSrc * 3)()
    for i, s in enumerate(srcs):
        t = s.t
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
            raise RuntimeError(f"nps_hip: sources must be contiguous fp32 NHWC, got {t.dtype} {tuple(t.shape)}")
        arr[i].ptr = ptr(t)
        arr[i].H, arr[i].W, arr[i].C = t.shape[1], t.shape[2], t.shape[3]
        arr[i].off_y, arr[i].off_x = int(s.off_y), int(s.off_x)
    return arr


def crop_offset(cur: int, des: int) -> int:
    """Top/left zero-pad (negative = crop) that crop_Nd applies when resizing cur -> des
    (models/common.py:20-34: the ±0.001 tie-break pads the trailing side one more)."""
    return int(round((des - cur) / 2 - 0.001))


def empty_nhwc(B, H, W, C, like: torch.Tensor):
    return torch.empty((B, H, W, C), dtype=torch.float32, device=like.device)


# ----------------------------------------------------------------- weights ----
def _pack(w, Cout, Cin, KH, KW, mode, precision):
    n = lib.nps_conv2d_packed_size(Cout, Cin, KH * KW)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    fn = lib.nps_conv2d_pack_weights_x3 if precision == PREC_X3F16 else lib.nps_conv2d_pack_weights
    check(fn(ptr(w), ptr(out), Cout, Cin, KH, KW, mode, stream_ptr()), "conv2d_pack_weights")
    out.nps_precision = precision   # read back by conv2d(): the kernel must match the packing
    # how to redo it in place (_repack_stale): the source pointer and the pack arguments (split-fp16 packings only)
    out._nps_job = (w.data_ptr(), Cout, Cin, KH, KW, mode) if precision == PREC_X3F16 else None
    return out


# After an optimizer step every cached packing is stale (trainers/base.py:493 bumps every parameter's version):
# the first stale lookup repacks ALL stale split-fp16 packings of the device in one batched call
# (nps_conv2d_pack_weights_x3_batch, two launches per 48 weights) into their existing buffers, instead of two
# launches per weight and kind (~430 per U-FNO training step, launch-bound).  Dev knob NPS_PACK_BATCH=0: off.
PACK_BATCH = os.environ.get("NPS_PACK_BATCH", "1") != "0"
_PACK_OWNERS = weakref.WeakValueDictionary()  # id(parameter) -> parameter holding a pack cache


def _pack_key(w):
    return (w.data_ptr(), w._version, str(w.device), CONV_PRECISION)


def _replay_jobs(w, packed):
    """The batch jobs that redo `packed` (one tensor or the convT phase list) from w in place, or None."""
    ts = packed if isinstance(packed, list) else [packed]
    jobs = []
    for t in ts:
        j = getattr(t, "_nps_job", None)
        if j is None or j[0] != w.data_ptr():
            return None
        jobs.append(PackJob(w.data_ptr(), t.data_ptr(), *j[1:]))
    return jobs


def _repack_stale(device):
    jobs, fresh = [], []
    for p in list(_PACK_OWNERS.values()):
        if p.device != device:
            continue
        key = _pack_key(p)
        for kind, (k, packed) in list(getattr(p, "_nps_packs", {}).items()):
            if k == key or k[3] != CONV_PRECISION:
                continue
            js = _replay_jobs(p, packed)
            if js is not None:
                jobs += js
                fresh.append((p, kind, key, packed))
    if jobs:
        check(lib.nps_conv2d_pack_weights_x3_batch((PackJob * len(jobs))(*jobs), len(jobs), stream_ptr()),
              "conv2d_pack_weights_x3_batch")
    for p, kind, key, packed in fresh:
        p._nps_packs[kind] = (key, packed)


def cached_pack(w: torch.Tensor, kind, fn):
    """fn(w) — a packed copy of the parameter w — cached on w per `kind` until w changes (data pointer,
    w._version: the optimizer's in-place step bumps it) or the conv precision does.  The inference run()
    paths and the autograd functions share the cache, so a training step packs each weight once for the
    no-grad pushforward unroll and the differentiable forward together; a stale entry first triggers the batched
    repack of every stale packing on the device (_repack_stale)."""
    key = _pack_key(w)
    cache = getattr(w, "_nps_packs", None)
    if cache is None:
        cache = w._nps_packs = {}
    ent = cache.get(kind)
    if ent is not None and ent[0] != key and PACK_BATCH and ent[0][3] == CONV_PRECISION:
        _repack_stale(w.device)
        ent = cache.get(kind)
    if ent is None or ent[0] != key:
        ent = cache[kind] = (key, fn(w))
        _PACK_OWNERS[id(w)] = w
    return ent[1]


def pack_conv_weight(w: torch.Tensor, stride=1, dil=1) -> torch.Tensor:
    """nn.Conv2d weight (Cout, Cin, KH, KW) -> MFMA-fragment-packed buffer (fp32 or split-fp16 fragments,
    whichever the conv of this geometry runs in)."""
    w = w.detach().contiguous()
    Cout, Cin, KH, KW = w.shape
    return _pack(w, Cout, Cin, KH, KW, -1, conv_precision(KH, KW, stride, dil))


def pack_conv_weight_dgrad(w: torch.Tensor, dil=1) -> torch.Tensor:
    """Weight (Cout, Cin, KH, KW) of a stride-1 conv -> the packed weight of its input-gradient conv
    (Cin outputs, Cout inputs, taps flipped): the transpose + flip happen inside the pack kernel (mode -3)."""
    w = w.detach().contiguous()
    Cout, Cin, KH, KW = w.shape
    return _pack(w, Cin, Cout, KH, KW, -3, conv_precision(KH, KW, 1, dil))


def pack_conv_weight_s2d(w: torch.Tensor) -> torch.Tensor:
    """3x3 stride-2 weight (Cout, C, 3, 3) -> packed 2x2 conv over the space-to-depth input (4C channels)."""
    w = w.detach().contiguous()
    Cout, C = w.shape[0], w.shape[1]
    return _pack(w, Cout, 4 * C, 2, 2, -2, conv_precision(2, 2))


def space_to_depth(x: torch.Tensor, pad: int, Hq: int, Wq: int) -> torch.Tensor:
    B, H, W, C = x.shape
    out = torch.empty((B, Hq, Wq, 4 * C), dtype=torch.float32, device=x.device)
    check(lib.nps_space_to_depth(ptr(x), ptr(out), B, H, W, C, pad, Hq, Wq, stream_ptr()), "space_to_depth")
    return share_tag(out, x)


def pack_convT_phases(w: torch.Tensor) -> List[torch.Tensor]:
    """nn.ConvTranspose2d(k=4, s=2) weight (Cin, Cout, 4, 4) -> 4 packed 2x2 phase convs, views of ONE buffer
    (phase ph at ph * nps_phase_stride floats), so the split-fp16 kernel can run all 4 in one launch
    (nps_conv2d_t.nphase, conv2d(phases=...))."""
    w = w.detach().contiguous()
    Cin, Cout = w.shape[0], w.shape[1]
    prec = conv_precision(2, 2)
    n = lib.nps_conv2d_packed_size(Cout, Cin, 4)
    buf = torch.cat([_pack(w, Cout, Cin, 2, 2, ph, prec) for ph in range(4)])
    views = []
    for ph in range(4):
        v = buf[ph * n:(ph + 1) * n]
        v.nps_precision = prec
        v.nps_phase_stride = n
        v._nps_job = (w.data_ptr(), Cout, Cin, 2, 2, ph) if prec == PREC_X3F16 else None
        views.append(v)
    return views


def pack_spectral_weight(w1: torch.Tensor, w2: torch.Tensor, H: int) -> torch.Tensor:
    """weights1/weights2 (Cin, Cout, m1, m2) complex64 -> [R][m2][Cin][Cout] complex for frame height H."""
    w1 = w1.detach().contiguous()
    w2 = w2.detach().contiguous()
    Cin, Cout, m1, m2 = w1.shape
    R = min(H, 2 * m1)
    out = torch.empty((R, m2, Cin, Cout), dtype=torch.complex64, device=w1.device)
    check(lib.nps_spectral_pack_weights(ptr(w1), ptr(w2), ptr(out), Cin, Cout, H, m1, m2, stream_ptr()),
          "spectral_pack_weights")
    return out


# ------------------------------------------------------------------- conv -----
class GN(NamedTuple):
    stats: torch.Tensor      # (B, G, 2) float64
    gamma: torch.Tensor
    beta: torch.Tensor
    groups: int
    eps: float


def _set_prologue(a, gn: Optional[GN], pre_act):
    """The GroupNorm + activation prologue fields of a Conv2dArgs / Conv3dArgs."""
    if gn is not None:
        a.gn_stats, a.gn_gamma, a.gn_beta = ptr(gn.stats), ptr(gn.gamma), ptr(gn.beta)
        a.gn_groups, a.gn_eps = gn.groups, gn.eps
    a.pre_act = pre_act


def group_norm_stats(srcs: Sequence[Src], frame_hw, groups: int) -> torch.Tensor:
    """(B, groups, 2) fp64 (sum, sum of squares) of the virtual frame's groups — the moments of
    nn.GroupNorm.  GroupNorm(1) of sources that each lie wholly inside the frame (crop_Nd zero-pads them,
    it does not cut them): the sum of the sources' carried moments (source_stats)."""
    t0 = srcs[0].t
    B = t0.shape[0]
    if groups == 1 and all(0 <= s.off_y and s.off_y + s.t.shape[1] <= frame_hw[0] and
                           0 <= s.off_x and s.off_x + s.t.shape[2] <= frame_hw[1] for s in srcs):
        parts = [source_stats(s.t) for s in srcs]
        if len(parts) == 1 and parts[0].shape[1] == 1:
            return parts[0]
        return _stats_sum(parts, B, new_stats(B, t0, 1))
    Cin = sum(s.t.shape[3] for s in srcs)
    if _DEBUG_STATS:
        import traceback
        print("nps stats pass (frame)", [tuple(s.t.shape) for s in srcs], frame_hw, groups,
              "".join(traceback.format_stack(limit=5)[:-1]), flush=True)
    stats = torch.empty((B, groups, 2), dtype=torch.float64, device=t0.device)
    check(lib.nps_group_norm_stats(_c_src(srcs), len(srcs), B, frame_hw[0], frame_hw[1], Cin, groups, ptr(stats), 1,
                                   stream_ptr()), "group_norm_stats")
    return stats


def conv2d(srcs: Sequence[Src], frame_hw, wpack: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, KH: int,
           KW: int, stride=1, dil=1, pad=(0, 0), circ=0, out_hw=None, gn: Optional[GN] = None, pre_act=0,
           out: Optional[torch.Tensor] = None, out_nchw=False, out_os=1, out_off=(0, 0), accumulate=False,
           addends: Sequence[torch.Tensor] = (), act=0, add_after_act=False, pad_bottom=None,
           in_scale: Optional[Union[torch.Tensor, int]] = None, out_stats: Optional[torch.Tensor] = None, phases: int = 1,
           s2d_pad: Optional[int] = None, spec: Optional[tuple] = None):
    """One fused conv launch.  `pad` = top/left zero padding (in the circularly
    extended frame), `pad_bottom` defaults to `pad`.  `out_stats`: a new_stats() buffer the launch adds
    the GroupNorm(1) moments of its stored values to (marked incomplete when this conv's kernel cannot;
    attach_stats then ignores it).  `phases` = 4: `wpack` is phase 0 of pack_convT_phases and the launch runs
    all 4 transposed-conv phases, phase (py, px) written at out_off + (py, px) (split-fp16 only).  `s2d_pad`:
    the frame (frame_hw, 4 C channels) is the space-to-depth view of the single source srcs[0] (C % 16 == 0)
    with that padding (nps_conv2d_t.s2d; the Downsample's 3x3/s2 conv as a 2x2 conv).  Returns `out`."""
    t0 = srcs[0].t
    B = t0.shape[0]
    Hin, Win = int(frame_hw[0]), int(frame_hw[1])
    Cin = sum(s.t.shape[3] for s in srcs)
    if s2d_pad is not None:
        if len(srcs) != 1 or Cin % 16 or gn is not None or pre_act or KH != 2 or KW != 2:
            raise ValueError("conv2d: the space-to-depth view takes one 16-channel-aligned source, a 2x2 kernel, "
                             "no prologue")
        Cin *= 4
    cin_alg = Cin  # algorithmic input channels (before any zero channel padding)
    x3 = getattr(wpack, "nps_precision", PREC_F32) == PREC_X3F16
    aligned = not x3 or lib.nps_conv2d_x3_sources_ok(_c_src(srcs), len(srcs))
    fused = (x3 and aligned and FUSE_PROLOGUE and (gn is not None or pre_act) and stride == 1 and dil == 1 and
             lib.nps_conv2d_x3_prologue_ok(KH, KW, Cin, gn.groups if gn is not None else 0, pre_act) and
             (KH * KW != 1 or (FUSE_PROLOGUE_1X1 and Cout <= 192 and not out_nchw and phases == 1)))
    if not fused and (((gn is not None or pre_act) and stride == 1 and dil == 1 and KH == KW and KH in (1, 2, 3))
                      or not aligned):
        # the stride-1 producer/consumer convs stage raw bytes only (the split-fp16 one from 16-channel
        # aligned sources): materialise act(GN(frame)) / the concatenation once
        srcs = [Src(frame_pack(srcs, (Hin, Win), gn, pre_act, pad4=x3))]
        gn, pre_act = None, 0
        Cin = srcs[0].t.shape[3]  # (channel padding: the packed weight is zero for ci >= the true Cin)
    pb = pad if pad_bottom is None else pad_bottom
    if out_hw is None:
        Hout = (Hin + 2 * circ + pad[0] + pb[0] - dil * (KH - 1) - 1) // stride + 1
        Wout = (Win + 2 * circ + pad[1] + pb[1] - dil * (KW - 1) - 1) // stride + 1
    else:
        Hout, Wout = out_hw
    if Hout <= 0 or Wout <= 0:
        raise RuntimeError(f"nps_hip conv2d: empty output {Hout}x{Wout} for input {Hin}x{Win} k={KH}")
    out_given = out is not None
    if out_given:
        drop_stats(out)
    if out is None:
        out = (torch.empty((B, Cout, Hout, Wout), dtype=torch.float32, device=t0.device) if out_nchw
               else empty_nhwc(B, Hout, Wout, Cout, t0))
    if out_nchw:
        oC, oH, oW = out.shape[1], out.shape[2], out.shape[3]
    else:
        oH, oW, oC = out.shape[1], out.shape[2], out.shape[3]
    a = Conv2dArgs()
    a.nsrc = len(srcs)
    a.src = _c_src(srcs)
    a.B, a.Hin, a.Win, a.Cin = B, Hin, Win, Cin
    if s2d_pad is not None:
        a.s2d, a.s2d_pad = 1, int(s2d_pad)
    _set_prologue(a, gn, pre_act)
    a.KH, a.KW, a.stride, a.dil = KH, KW, stride, dil
    a.pad_y, a.pad_x, a.circ = pad[0], pad[1], circ
    a.Hout, a.Wout = Hout, Wout
    a.wpack, a.bias, a.Cout = ptr(wpack), ptr(bias), Cout
    a.out, a.out_C, a.out_H, a.out_W = ptr(out), oC, oH, oW
    a.out_os, a.out_off_y, a.out_off_x = out_os, out_off[0], out_off[1]
    a.out_nchw = 1 if out_nchw else 0
    a.accumulate = 1 if accumulate else 0
    ads = list(addends)
    a.addend0 = ptr(ads[0]) if len(ads) > 0 else None
    a.addend1 = ptr(ads[1]) if len(ads) > 1 else None
    a.act, a.add_after_act = act, (1 if add_after_act else 0)
    a.precision = getattr(wpack, "nps_precision", PREC_F32)
    if spec is not None:  # (Z, m2, scale): the spectral conv's W pass added in the epilogue (spectral_fusable)
        Z, m2s, sc = spec
        if Z.dtype != torch.complex64 or not Z.is_contiguous() or tuple(Z.shape) != (B, Hout, m2s, Cout):
            raise RuntimeError("conv2d: spec Z must be contiguous complex64 (B, Hout, m2, Cout)")
        a.spec_z, a.spec_m2, a.spec_scale = ptr(Z), m2s, float(sc)
    if phases > 1:
        if a.precision != PREC_X3F16 or phases != 4 or out_os != 2:
            raise ValueError("conv2d: merged transposed-conv phases need the split-fp16 2x2 packing and out_os 2")
        a.nphase, a.phase_wstride = 4, wpack.nps_phase_stride
    reserve_tags(out.device, len(srcs) + 1)  # every tag this launch reads or writes, before any pointer
    if a.precision == PREC_X3F16:
        if in_scale is not None:  # explicit range (a tag tensor or its device pointer): overrides the sources' tags
            a.in_scale = in_scale if isinstance(in_scale, int) else ptr(in_scale)
        elif USE_IN_TAGS and not (fused and gn is not None):
            # the sources' tags (a fused GroupNorm prologue normalises the frame: its output range is not
            # the sources'; the kernel bounds it from gamma, beta and the group size, gn_prologue_scale)
            tags = [input_tag(s.t) for s in srcs] + [None, None]
            a.in_scale, a.in_tag1, a.in_tag2 = tags[0], tags[1], tags[2]
    if USE_OUT_TAGS:
        a.out_tag = out_tag(out, accumulate) if out_given else new_tag(out)
    if out_stats is not None:
        # 1x1: the LDS-weight kernel's fused epilogue (at most one addend, no accumulate) takes the moments of the
        # stored values, activation and addend included
        plain = not accumulate and len(ads) <= 1
        x1_ok = Cout <= 192 and plain
        if (a.precision == PREC_X3F16 and (KH * KW != 1 or x1_ok)
                and not out_nchw and oC % 4 == 0 and Cout % 4 == 0):
            a.out_stats = ptr(out_stats)
        else:
            out_stats._nps_incomplete = True
    if lib.nps_conv2d_plan(ctypes_byref(a)) < 0:
        raise RuntimeError("conv2d_plan failed: " + lib.nps_last_error().decode())
    if conv_probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.nps_conv2d_fwd(ctypes_byref(a), stream_ptr()), "conv2d_fwd")
        e1.record()
        nph = max(phases, 1)
        nbytes = 4.0 * (sum(s.t.numel() for s in srcs) + nph * (Cout * cin_alg * KH * KW + B * Hout * Wout * Cout))
        conv_probe.append((e0, e1, 2.0 * nph * B * Hout * Wout * Cout * cin_alg * KH * KW,
                           ("x3f16" if a.precision == PREC_X3F16 else "f32", KH * KW, a.waves), nbytes))
        if conv_shape_log is not None:
            conv_shape_log.append(dict(cin=cin_alg, cout=Cout, k=(KH, KW), hw=(Hin, Win), out=(Hout, Wout), B=B,
                                       nsrc=len(srcs), acc=bool(accumulate), addends=len(ads), act=act,
                                       gn=gn is not None, pre_act=pre_act, stats=out_stats is not None))
    else:
        check(lib.nps_conv2d_fwd(ctypes_byref(a), stream_ptr()), "conv2d_fwd")
    return out


def absmax(x: torch.Tensor) -> torch.Tensor:
    """Range tag (TAG_FLOATS fp32 device tensor, value max|x|) — the input range of a split-fp16 conv
    (conv2d(in_scale=...)); tag_value() reads it back."""
    x = x.contiguous()
    out = torch.empty(TAG_FLOATS, dtype=torch.float32, device=x.device)
    check(lib.nps_absmax(ptr(x), x.numel(), ptr(out), stream_ptr()), "absmax")
    return out


def tag_value(tag) -> float:
    """Host value of a range tag (a tag tensor, or a tensor carrying a live tag) — for tests / diagnostics."""
    if isinstance(tag, torch.Tensor) and tag.numel() == TAG_FLOATS and tag_of(tag) is None:
        return float(tag.view(64, 64)[:, 0].max())
    t = tag_of(tag)
    if t is None:
        return float("nan")
    i = (t.ptr - t.arena.buf.data_ptr()) // 4
    return float(t.arena.buf[i:i + TAG_FLOATS].view(64, 64)[:, 0].max())


def frame_pack(srcs: Sequence[Src], frame_hw, gn: Optional[GN] = None, pre_act=0, pad4=False) -> torch.Tensor:
    """(B, Hin, Win, Cin) = act(GN(virtual frame)) — nps_frame_pack; pad4: channels zero-padded to a
    multiple of 4 (the split-fp16 conv stages 16-B channel groups)."""
    t0 = srcs[0].t
    B = t0.shape[0]
    Hin, Win = int(frame_hw[0]), int(frame_hw[1])
    Cin = sum(s.t.shape[3] for s in srcs)
    a = Conv2dArgs()
    a.nsrc = len(srcs)
    a.src = _c_src(srcs)
    a.B, a.Hin, a.Win, a.Cin = B, Hin, Win, Cin
    _set_prologue(a, gn, pre_act)
    a.out_C = (Cin + 3) // 4 * 4 if pad4 else Cin
    out = empty_nhwc(B, Hin, Win, a.out_C, t0)
    a.out_tag = new_tag(out)
    check(lib.nps_frame_pack(ctypes_byref(a), ptr(out), stream_ptr()), "frame_pack")
    return out


def ctypes_byref(x):
    import ctypes
    return ctypes.byref(x)


# --------------------------------------------------------------- spectral -----
def _film_operands(film, B: int, N: int):
    """film = (p (B, K), weights_feat.weight (N, K), weights_feat.bias (N,), transform_mode) checked (fp32 device
    tensors of these shapes) and returned detached and contiguous."""
    p, Wf, bf, mode = film
    for t in (p, Wf, bf):
        ptr(t)  # no CPU path
        if t.dtype != torch.float32:
            raise TypeError(f"FiLM operands are fp32 tensors, got {t.dtype}")
    if p.dim() != 2 or p.shape[0] != B or tuple(Wf.shape) != (N, p.shape[1]) or tuple(bf.shape) != (N,):
        raise ValueError(f"FiLM shapes: p (B={B}, K), weights_feat.weight ({N}, K), bias ({N},); got "
                         f"{tuple(p.shape)}, {tuple(Wf.shape)}, {tuple(bf.shape)}")
    return p.detach().contiguous(), Wf.detach().contiguous(), bf.detach().contiguous(), mode


def film_scale(film, B: int, Cout: int, H: int, m1: int, m2: int) -> torch.Tensor:
    """The FiLM factor S (B, R, m2, Cout) fp32 of the retained modes (proc_fno.py:271-284; include/nps.h,
    nps_spectral_film_scale) from film = (p (B, K), weights_feat.weight (Cout*2*m1*m2, K), weights_feat.bias,
    transform_mode)."""
    p, Wf, bf, mode = _film_operands(film, B, Cout * 2 * m1 * m2)
    S = torch.empty((B, min(H, 2 * m1), m2, Cout), dtype=torch.float32, device=p.device)
    check(lib.nps_spectral_film_scale(ptr(p), ptr(Wf), ptr(bf), ptr(S), B, p.shape[1], Cout, H, m1, m2, int(mode),
                                      stream_ptr()), "spectral_film_scale")
    return S


def spectral_mix(X2, wpack, Y, B, R, m2, Cin, Cout, S=None):
    """Y = the per-mode channel mixing of X2 (times the FiLM factor S in the store, when given)."""
    if S is None:
        check(lib.nps_spectral_mix(ptr(X2), ptr(wpack), ptr(Y), B, R, m2, Cin, Cout, stream_ptr()), "spectral_mix")
    else:
        check(lib.nps_spectral_mix_scaled(ptr(X2), ptr(wpack), ptr(S), ptr(Y), B, R, m2, Cin, Cout, stream_ptr()),
              "spectral_mix_scaled")


# The W passes are the only stages of a spectral conv that see the activation layout (csrc/spectral_abi.hip: Lay and
# w_dft ... w_dft_bwd).  One adapter per layout issues them; spectral2d_fwd / spectral3d_fwd here and the backward
# chains of autograd.py hold the stage order once and take an adapter.  `dims` is (B, H, W, Cin) of the input as the
# W pass sees it (H = D*H rows in 3-D); the backward passes need no input, so they hang off the class.
class NhwcW:
    """fp32 NHWC sources covering a virtual frame (Sequence[Src])."""
    out_dtype = torch.float32

    def __init__(self, srcs: Sequence[Src]):
        t0 = srcs[0].t
        self.srcs, self.device = srcs, t0.device
        self.dims = (t0.shape[0], t0.shape[1], t0.shape[2], sum(s.t.shape[3] for s in srcs))

    @classmethod
    def of(cls, x: torch.Tensor):
        """The adapter of one whole tensor (the autograd Functions' input)."""
        return cls([Src(x.contiguous())])

    def new_out(self, Cout):
        B, H, W, _ = self.dims
        return torch.empty((B, H, W, Cout), dtype=self.out_dtype, device=self.device)

    def dft_w(self, m, X1):
        B, H, W, Cin = self.dims
        check(lib.nps_spectral_dft_w(_c_src(self.srcs), len(self.srcs), B, H, W, Cin, m, ptr(X1), stream_ptr()),
              "spectral_dft_w")

    def idft_w(self, Z, out, m, Cout, accumulate=False, act=0, addend=None):
        """out (= or +=) act(W synthesis of Z + addend); raises out's range tag (a fresh one on a new tensor)."""
        B, H, W, _ = self.dims
        check(lib.nps_spectral_idft_w(ptr(Z), ptr(out), B, H, W, m, Cout, 1 if accumulate else 0, ptr(addend), act,
                                      out_tag(out, accumulate), stream_ptr()), "spectral_idft_w")

    @staticmethod
    def idft_w_bwd(gy, gZ, B, H, W, m, Cout):
        check(lib.nps_spectral_idft_w_bwd(ptr(gy.contiguous()), ptr(gZ), B, H, W, m, Cout, stream_ptr()),
              "spectral_idft_w_bwd")

    @staticmethod
    def dft_w_bwd(gX1, B, H, W, m, Cin):
        dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=gX1.device)
        check(lib.nps_spectral_dft_w_bwd(ptr(gX1), ptr(dx), B, H, W, m, Cin, stream_ptr()), "spectral_dft_w_bwd")
        return dx


class NchwW:
    """One fp32 channels-first tensor (B, C, *spatial), read as it lies with its batch stride (channels_first)."""

    def __init__(self, x: torch.Tensor):
        self.x, self.x_bs = channels_first(x)
        B, Cin, W = self.x.shape[0], self.x.shape[1], self.x.shape[-1]
        self.device = self.x.device
        self.dims = (B, self.x[0, 0].numel() // W, W, Cin)

    @classmethod
    def of(cls, x: torch.Tensor):
        return cls(x)

    def new_out(self, Cout):
        return torch.empty((self.x.shape[0], Cout) + tuple(self.x.shape[2:]), dtype=torch.float32, device=self.device)

    def dft_w(self, m, X1):
        B, H, W, Cin = self.dims
        check(lib.nps_spectral_dft_w_nchw(ptr(self.x), self.x_bs, B, H, W, Cin, m, ptr(X1), stream_ptr()),
              "spectral_dft_w_nchw")

    def idft_w(self, Z, out, m, Cout, accumulate=False, act=0, out_bs=0):
        B, H, W, _ = self.dims
        check(lib.nps_spectral_idft_w_nchw(ptr(Z), ptr(out), out_bs, B, H, W, m, Cout, 1 if accumulate else 0, act,
                                           stream_ptr()), "spectral_idft_w_nchw")

    @staticmethod
    def idft_w_bwd(gy, gZ, B, H, W, m, Cout):
        gy, gy_bs = channels_first(gy)
        check(lib.nps_spectral_idft_w_bwd_nchw(ptr(gy), gy_bs, ptr(gZ), B, H, W, m, Cout, stream_ptr()),
              "spectral_idft_w_bwd_nchw")

    @staticmethod
    def dft_w_bwd(gX1, B, H, W, m, Cin):
        dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gX1.device)
        check(lib.nps_spectral_dft_w_bwd_nchw(ptr(gX1), ptr(dx), 0, B, H, W, m, Cin, stream_ptr()),
              "spectral_dft_w_bwd_nchw")
        return dx


class Bf16W(NhwcW):
    """bf16 NHWC sources and output, fp32 spectra; forward only."""
    out_dtype = torch.bfloat16
    idft_w_bwd = dft_w_bwd = None

    def dft_w(self, m, X1):
        B, H, W, Cin = self.dims
        check(lib.nps_spectral_dft_w_bf16(_c_src_bf16(self.srcs), len(self.srcs), B, H, W, Cin, m, ptr(X1),
                                          stream_ptr()), "spectral_dft_w_bf16")

    def idft_w(self, Z, out, m, Cout, accumulate=False, act=0, addend=None):
        B, H, W, _ = self.dims
        check(lib.nps_spectral_idft_w_bf16(ptr(Z), ptr(out), B, H, W, m, Cout, 1 if accumulate else 0, ptr(addend),
                                           act, stream_ptr()), "spectral_idft_w_bf16")


def spectral2d_fwd(lay, wpack: torch.Tensor, m1: int, m2: int, Cout: int, film=None):
    """The SpectralConv2d forward up to its W-pass synthesis (proc_fno.py:257-288): W and H analysis on the retained
    modes, the mode mixing (times the FiLM factor of film = (p, Wf, bf, transform_mode), film_scale), the inverse H
    pass.  Returns (X2 (B, R, m2, Cin) kept for the backward, Z (B, H, m2, Cout) for lay.idft_w, S or None)."""
    B, H, W, Cin = lay.dims
    if not (m1 <= H and m2 <= W // 2 + 1):
        raise AssertionError("modes should be at most the spatial dim (// 2 + 1 for the last spatial dimension)")
    S = film_scale(film, B, Cout, H, m1, m2) if film is not None else None
    R = min(H, 2 * m1)
    X1 = torch.empty((B, H, m2, Cin), dtype=torch.complex64, device=lay.device)
    X2 = torch.empty((B, R, m2, Cin), dtype=torch.complex64, device=lay.device)
    Y = torch.empty((B, R, m2, Cout), dtype=torch.complex64, device=lay.device)
    Z = torch.empty((B, H, m2, Cout), dtype=torch.complex64, device=lay.device)
    s = stream_ptr()
    lay.dft_w(m2, X1)
    check(lib.nps_spectral_dft_h(ptr(X1), ptr(X2), B, H, m1, m2, Cin, s), "spectral_dft_h")
    spectral_mix(X2, wpack, Y, B, R, m2, Cin, Cout, S)
    check(lib.nps_spectral_idft_h(ptr(Y), ptr(Z), B, H, m1, m2, Cout, s), "spectral_idft_h")
    return X2, Z, S


def spectral_z(srcs: Sequence[Src], wpack: torch.Tensor, m1: int, m2: int, Cout: int, film=None) -> torch.Tensor:
    """Z (B, H, m2, Cout) complex64: the spectral conv up to its W-pass synthesis (spectral2d_fwd) — spectral_conv2d's
    idft_w input, or the spec_z a 1x1 conv's epilogue synthesises itself (conv2d(spec=...), the FNO layer fusion)."""
    return spectral2d_fwd(NhwcW(srcs), wpack, m1, m2, Cout, film=film)[1]


# the FNO layer's 1x1 `w` synthesises the spectral conv's W pass in its epilogue (nps_conv2d_t.spec_z) instead of a
# separate idft_w read-modify-write of its output (dev knob NPS_FUSE_IDFT=0: off)
FUSE_IDFT = os.environ.get("NPS_FUSE_IDFT", "1") != "0"


def spectral_fusable(W: int, m2: int, Cout: int) -> bool:
    """Whether conv2d(spec=...) can take this spectral conv's W pass (nps_conv2d_t.spec_z conditions)."""
    return (FUSE_IDFT and CONV_PRECISION == PREC_X3F16 and W % 128 == 0 and m2 <= 16
            and Cout <= 192 and Cout % 4 == 0)


def spectral_conv2d(srcs: Sequence[Src], wpack: torch.Tensor, m1: int, m2: int, Cout: int,
                    out: Optional[torch.Tensor] = None, accumulate=False, addend=None, act=0, film=None):
    """y = irfft2(P(rfft2(x))) on the retained modes (proc_fno.py:257-288), NHWC in/out; film as in spectral2d_fwd."""
    lay = NhwcW(srcs)
    Z = spectral2d_fwd(lay, wpack, m1, m2, Cout, film=film)[1]
    if out is not None:
        drop_stats(out)
    if out is None:
        out = lay.new_out(Cout)
        accumulate = False
    lay.idft_w(Z, out, m2, Cout, accumulate, act, addend)
    return out


# ------------------------------------------------------------ spectral, 1-D -----
SPECTRAL1D_MAX_MODES = 128    # include/nps.h, SpectralConv1d envelope
SPECTRAL1D_MAX_L = 65536


def check_modes1d(L: int, m: int):
    """The SpectralConv1d envelope (mirrors the library's host checks)."""
    if not m <= L // 2 + 1:
        raise AssertionError("modes should be at most the spatial dim // 2 + 1 for the last spatial dimension!")
    if not (2 <= L <= SPECTRAL1D_MAX_L and 1 <= m <= SPECTRAL1D_MAX_MODES):
        raise NotImplementedError(f"SpectralConv1d on the MI355X path: 2 <= L <= {SPECTRAL1D_MAX_L} and 1 <= modes <= "
                                  f"{SPECTRAL1D_MAX_MODES}, got L={L} modes={m}")


def pack_spectral1d_weight(w: torch.Tensor) -> torch.Tensor:
    """weights1 (Cin, Cout, m) complex64 -> [m][Cin][Cout] complex (the mixer's packing with R = 1)."""
    w = w.detach().contiguous()
    Cin, Cout, m = w.shape
    out = torch.empty((m, Cin, Cout), dtype=torch.complex64, device=w.device)
    check(lib.nps_spectral1d_pack_weights(ptr(w), ptr(out), Cin, Cout, m, stream_ptr()), "spectral1d_pack_weights")
    return out


def _src1d(srcs: Sequence[Src]):
    """(B, L, C) sources as the (B, 1, L, C) frames the C ABI takes."""
    return _c_src([Src(s.t.unsqueeze(1) if s.t.dim() == 3 else s.t, s.off_y, s.off_x) for s in srcs])


def spectral1d_dft(srcs: Sequence[Src], m: int, adjoint=False) -> torch.Tensor:
    """X (B, m, C) complex64 = the first m bins of the DFT along L of the concatenated (B, L, C) sources (never
    materialised); adjoint: scaled by c_k / L, the adjoint of spectral1d_idft's synthesis."""
    t0 = srcs[0].t
    B, L = t0.shape[0], t0.shape[-2]
    C = sum(s.t.shape[-1] for s in srcs)
    arr = _src1d(srcs)
    check_modes1d(L, m)
    X = torch.empty((B, m, C), dtype=torch.complex64, device=t0.device)
    n = lib.nps_spectral1d_dft_workspace(B, L, C, m)
    ws = torch.empty((max(n, 4) // 4,), dtype=torch.float32, device=t0.device)
    check(lib.nps_spectral1d_dft(arr, len(srcs), B, L, C, m, ptr(X), ptr(ws), 1 if adjoint else 0, stream_ptr()),
          "spectral1d_dft")
    return X


def spectral1d_idft(Z: torch.Tensor, L: int, out: Optional[torch.Tensor] = None, accumulate=False, addend=None, act=0,
                    adjoint=False) -> torch.Tensor:
    """out (B, L, Cout) (= or +=) act(c2r_L(Z) / L + addend) from Z (B, m, Cout) complex64; adjoint: the analysis
    adjoint (no doubling, no 1 / L).  `out` may be any contiguous tensor of B * L * Cout floats."""
    B, m, Cout = Z.shape
    check_modes1d(L, m)
    if out is None:
        out = torch.empty((B, L, Cout), dtype=torch.float32, device=Z.device)
        accumulate = False
    else:
        drop_stats(out)
        out._nps_tag = None  # the synthesis publishes no range tag: readers measure the tensor again
    check(lib.nps_spectral1d_idft(ptr(Z), ptr(out), B, L, m, Cout, 1 if accumulate else 0, ptr(addend), act,
                                  1 if adjoint else 0, stream_ptr()), "spectral1d_idft")
    return out


def film1d_scale(film, B: int, Cout: int, m: int) -> torch.Tensor:
    """The FiLM factor S (B, m, Cout) fp32 (proc_fno.py:209-218) from film = (p (B, K), weights_feat.weight
    (Cout*m, K), weights_feat.bias, transform_mode)."""
    p, Wf, bf, mode = _film_operands(film, B, Cout * m)
    S = torch.empty((B, m, Cout), dtype=torch.float32, device=p.device)
    check(lib.nps_spectral1d_film_scale(ptr(p), ptr(Wf), ptr(bf), ptr(S), B, p.shape[1], Cout, m, int(mode),
                                        stream_ptr()), "spectral1d_film_scale")
    return S


def spectral1d_mid(srcs: Sequence[Src], wpack: torch.Tensor, m: int, Cout: int, film=None):
    """(X, Y, S): the retained spectrum of the sources, the mixed (and FiLM-scaled) modes, the FiLM factor."""
    X = spectral1d_dft(srcs, m)
    B, _, Cin = X.shape
    S = film1d_scale(film, B, Cout, m) if film is not None else None
    Y = torch.empty((B, m, Cout), dtype=torch.complex64, device=X.device)
    spectral_mix(X, wpack, Y, B, 1, m, Cin, Cout, S)
    return X, Y, S


def spectral_conv1d(srcs: Sequence[Src], wpack: torch.Tensor, m: int, Cout: int, out: Optional[torch.Tensor] = None,
                    accumulate=False, addend=None, act=0, film=None) -> torch.Tensor:
    """y = irfft(P(rfft(x))) on the retained modes (proc_fno.py:199-222), channels-last (B, L, C) in / out (or the
    (B, 1, L, C) view the 1x1 conv takes); film as in film1d_scale."""
    L = srcs[0].t.shape[-2]
    _, Y, _ = spectral1d_mid(srcs, wpack, m, Cout, film=film)
    return spectral1d_idft(Y, L, out=out, accumulate=accumulate, addend=addend, act=act)


def pack_spectral3d_weight(ws: Sequence[torch.Tensor], D: int, H: int) -> torch.Tensor:
    """SpectralConv3d weights1..4 (Cin, Cout, m1, m2, m3) complex64 -> wpack [R1][R2][m3][Cin][Cout]."""
    w1, w2, w3, w4 = [w.detach().contiguous() for w in ws]
    Cin, Cout, m1, m2, m3 = w1.shape
    R1, R2 = min(D, 2 * m1), min(H, 2 * m2)
    out = torch.empty((R1, R2, m3, Cin, Cout), dtype=torch.complex64, device=w1.device)
    check(lib.nps_spectral3d_pack_weights(ptr(w1), ptr(w2), ptr(w3), ptr(w4), ptr(out), Cin, Cout, D, H, m1, m2, m3,
                                          stream_ptr()), "spectral3d_pack_weights")
    return out


def check_modes3d(D, H, W, m1, m2, m3):
    """proc_fno.py:134-139 for three spatial dims."""
    if not (m1 <= D and m2 <= H and m3 <= W // 2 + 1):
        raise AssertionError("modes should be at most the spatial dim (// 2 + 1 for the last spatial dimension)")


def spectral3d_fwd(lay, D: int, wpack, m1, m2, m3, Cout, out, accumulate=False, act=0, mix=lib.nps_spectral_mix,
                   **last):
    """The SpectralConv3d forward chain (proc_fno.py:334-376), axis by axis with the 2-D kernels, on a (B, D, H, W)
    volume whose W passes `lay` issues on D*H rows; `mix` is the mixer of wpack's dtype, `last` what lay.idft_w takes
    beyond (accumulate, act).  Writes `out`; returns the X3 spectrum (kept for the backward)."""
    B, DH, W, Cin = lay.dims
    H = DH // D
    check_modes3d(D, H, W, m1, m2, m3)
    R1, R2 = min(D, 2 * m1), min(H, 2 * m2)
    dev = lay.device
    c64 = torch.complex64
    X1 = torch.empty((B, D * H, m3, Cin), dtype=c64, device=dev)
    X2 = torch.empty((B * D, R2, m3, Cin), dtype=c64, device=dev)
    X3 = torch.empty((B, R1, R2 * m3, Cin), dtype=c64, device=dev)
    Y = torch.empty((B, R1, R2 * m3, Cout), dtype=c64, device=dev)
    Z1 = torch.empty((B, D, R2 * m3, Cout), dtype=c64, device=dev)
    Z2 = torch.empty((B * D, H, m3, Cout), dtype=c64, device=dev)
    s = stream_ptr()
    lay.dft_w(m3, X1)
    check(lib.nps_spectral_dft_h(ptr(X1), ptr(X2), B * D, H, m2, m3, Cin, s), "spectral3d dft_h (H)")
    check(lib.nps_spectral_dft_h(ptr(X2), ptr(X3), B, D, m1, R2 * m3, Cin, s), "spectral3d dft_h (D)")
    check(mix(ptr(X3), ptr(wpack), ptr(Y), B, R1, R2 * m3, Cin, Cout, s), "spectral3d mix")
    check(lib.nps_spectral_idft_h(ptr(Y), ptr(Z1), B, D, m1, R2 * m3, Cout, s), "spectral3d idft_h (D)")
    check(lib.nps_spectral_idft_h(ptr(Z1), ptr(Z2), B * D, H, m2, m3, Cout, s), "spectral3d idft_h (H)")
    lay.idft_w(Z2, out, m3, Cout, accumulate, act, **last)
    return X3


def _spectral_conv3d(lay, mix, D, wpack, m1, m2, m3, Cout, out, accumulate, addend, act):
    """spectral_conv3d / _bf16 on their adapter: NHWC out handling around spectral3d_fwd."""
    if out is not None:
        drop_stats(out)
    if out is None:
        out = lay.new_out(Cout)
        accumulate = False
    spectral3d_fwd(lay, D, wpack, m1, m2, m3, Cout, out, accumulate, act, mix=mix, addend=addend)
    return out


def spectral_conv3d(srcs: Sequence[Src], D: int, wpack: torch.Tensor, m1: int, m2: int, m3: int, Cout: int,
                    out: Optional[torch.Tensor] = None, accumulate=False, addend=None, act=0):
    """y = irfftn(P(rfftn(x))) on the 4 retained corners (proc_fno.py:334-376).  Sources are NDHWC
    tensors viewed as (B, D*H, W, C); returns (B, D*H, W, Cout) (view it as (B, D, H, W, Cout))."""
    return _spectral_conv3d(NhwcW(srcs), lib.nps_spectral_mix, D, wpack, m1, m2, m3, Cout, out, accumulate, addend,
                            act)


# ------------------------------------------------- channels-first spectral convs -----
def channels_first(x: torch.Tensor):
    """(x, batch stride in elements) for the channels-first kernels: an fp32 ROCm tensor whose inner (C, *spatial)
    block is contiguous is passed as it lies (a channel slice of a larger tensor keeps its batch stride); anything
    else is made contiguous first."""
    ptr(x)  # no CPU path
    if x.dtype != torch.float32:
        raise TypeError(f"channels-first spectral convs take fp32 tensors, got {x.dtype}")
    inner = x[0].numel()
    if not (x[0].is_contiguous() and (x.shape[0] == 1 or x.stride(0) >= inner)):
        x = x.contiguous()
    return x, (0 if x.shape[0] == 1 else x.stride(0))


def _out_channels_first(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device), 0, False
    o, obs = channels_first(out)
    if o is not out or tuple(out.shape) != tuple(shape):
        raise ValueError("out must be an fp32 channels-first tensor of the result's shape with a contiguous "
                         "(C, *spatial) block")
    return out, obs, True


def spectral_conv2d_nchw(x: torch.Tensor, wpack: torch.Tensor, m1: int, m2: int, Cout: int,
                         out: Optional[torch.Tensor] = None, accumulate=False, act=0, film=None):
    """y = irfft2(P(rfft2(x))) on the retained modes (proc_fno.py:257-288), NCHW in / out with no transpose: x
    (B, Cin, H, W) -> (B, Cout, H, W); out (= or +=, then act) may be a channel slice of a larger tensor; film as in
    spectral2d_fwd."""
    lay = NchwW(x)
    B, H, W, _ = lay.dims
    out, out_bs, given = _out_channels_first(out, (B, Cout, H, W), lay.x)
    Z = spectral2d_fwd(lay, wpack, m1, m2, Cout, film=film)[1]
    lay.idft_w(Z, out, m2, Cout, accumulate and given, act, out_bs)
    return out


def spectral_conv3d_nchw(x: torch.Tensor, wpack: torch.Tensor, m1: int, m2: int, m3: int, Cout: int,
                         out: Optional[torch.Tensor] = None, accumulate=False, act=0):
    """y = irfftn(P(rfftn(x))) on the 4 retained corners (proc_fno.py:334-376), NCDHW in / out with no transpose:
    x (B, Cin, D, H, W) -> (B, Cout, D, H, W)."""
    lay = NchwW(x)
    B, _, D, H, W = lay.x.shape
    out, out_bs, given = _out_channels_first(out, (B, Cout, D, H, W), lay.x)
    spectral3d_fwd(lay, D, wpack, m1, m2, m3, Cout, out, accumulate and given, act, out_bs=out_bs)
    return out


# ------------------------------------------------------------------ bf16 storage (C5) -----
def _c_src_bf16(srcs: Sequence[Src]):
    arr = (_CSrc * 3)()
    for i, s in enumerate(srcs):
        t = s.t
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.dim() != 4:
            raise RuntimeError(f"nps_hip: bf16 sources must be contiguous bf16 NHWC, got {t.dtype} {tuple(t.shape)}")
        arr[i].ptr = ptr(t)
        arr[i].H, arr[i].W, arr[i].C = t.shape[1], t.shape[2], t.shape[3]
        arr[i].off_y, arr[i].off_x = int(s.off_y), int(s.off_x)
    return arr


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 copy (round-to-nearest-even) of an fp32 (or complex64, as its (re, im) pairs) device tensor."""
    if x.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"nps_hip to_bf16: expected float32 or complex64, got {x.dtype}")
    x = x.contiguous()
    xf = torch.view_as_real(x) if x.is_complex() else x
    out = torch.empty(xf.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.nps_f32_to_bf16(ptr(xf), xf.numel(), ptr(out), stream_ptr()), "f32_to_bf16")
    return out


def to_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 copy of a bf16 device tensor."""
    if x.dtype != torch.bfloat16:
        raise TypeError(f"nps_hip to_f32: expected bfloat16, got {x.dtype}")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib.nps_bf16_to_f32(ptr(x), x.numel(), ptr(out), stream_ptr()), "bf16_to_f32")
    return out


def pack_1x1_bf16(w: torch.Tensor) -> torch.Tensor:
    """Pointwise conv weight (Cout, Cin[, 1...]) fp32 -> the bf16 [Cout][KR] packing of nps_conv1x1_bf16."""
    w = w.detach().reshape(w.shape[0], w.shape[1]).contiguous()
    Cout, Cin = w.shape
    out = torch.empty(Cout * lib.nps_conv1x1_bf16_kr(Cin), dtype=torch.bfloat16, device=w.device)
    check(lib.nps_pack_1x1_bf16(ptr(w), ptr(out), Cout, Cin, stream_ptr()), "pack_1x1_bf16")
    return out


def conv1x1_bf16(srcs: Sequence[Src], wpack: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, act=0,
                 addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(w x + bias [+ addend]) of a bf16 NHWC virtual frame (sources covering it) -> bf16 (B, H, W, Cout)."""
    t0 = srcs[0].t
    B, H, W = t0.shape[0], t0.shape[1], t0.shape[2]
    a = Conv2dArgs()
    a.nsrc = len(srcs)
    a.src = _c_src_bf16(srcs)
    a.B, a.Hin, a.Win, a.Cin = B, H, W, sum(s.t.shape[3] for s in srcs)
    a.KH = a.KW = a.stride = a.dil = 1
    a.Hout, a.Wout = H, W
    a.wpack, a.bias, a.Cout = ptr(wpack), ptr(bias), Cout
    out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=t0.device)
    a.out, a.out_C, a.out_H, a.out_W, a.out_os = ptr(out), Cout, H, W, 1
    a.addend0 = ptr(addend)
    a.act = act
    check(lib.nps_conv1x1_bf16(ctypes_byref(a), stream_ptr()), "conv1x1_bf16")
    return out


def spectral_conv3d_bf16(srcs: Sequence[Src], D: int, wpack_bf16: torch.Tensor, m1: int, m2: int, m3: int, Cout: int,
                         out: Optional[torch.Tensor] = None, accumulate=False, addend=None, act=0):
    """spectral_conv3d with bf16 activations in / out and bf16 packed weights (fp32 spectra and sums)."""
    return _spectral_conv3d(Bf16W(srcs), lib.nps_spectral_mix_bf16, D, wpack_bf16, m1, m2, m3, Cout, out, accumulate,
                            addend, act)


# ------------------------------------------------------------ 3-D U-Net (C5) -----
class Src3(NamedTuple):
    t: torch.Tensor          # (B, D, H, W, C) NDHWC contiguous, fp32 or bf16
    off_d: int = 0
    off_h: int = 0
    off_w: int = 0


def _fill_frame3(a, srcs: Sequence[Src3], frame_dhw):
    t0 = srcs[0].t
    dt = t0.dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"nps_hip conv3d: fp32 or bf16 sources, got {dt}")
    a.nsrc = len(srcs)
    for i, s in enumerate(srcs):
        t = s.t
        if t.dtype != dt or not t.is_contiguous() or t.dim() != 5 or t.shape[0] != t0.shape[0]:
            raise RuntimeError(f"nps_hip conv3d: sources must be contiguous NDHWC of one dtype / batch, got "
                               f"{t.dtype} {tuple(t.shape)}")
        a.src[i].ptr = ptr(t)
        a.src[i].D, a.src[i].H, a.src[i].W, a.src[i].C = t.shape[1], t.shape[2], t.shape[3], t.shape[4]
        a.src[i].off_d, a.src[i].off_h, a.src[i].off_w = int(s.off_d), int(s.off_h), int(s.off_w)
    a.B = t0.shape[0]
    a.Dc, a.Hc, a.Wc = (int(v) for v in frame_dhw)
    a.Cin = sum(s.t.shape[4] for s in srcs)
    a.bf16 = 1 if dt == torch.bfloat16 else 0
    return a


def pack_conv3d_weight(w: torch.Tensor, transposed=False, bf16=False) -> torch.Tensor:
    """nn.Conv3d weight (Cout, Cin, K, K, K) / nn.ConvTranspose3d weight (Cin, Cout, 4, 4, 4) -> the
    nps_conv3d packing in fp32 or bf16."""
    w = w.detach().float().contiguous()
    if transposed:
        Cin, Cout, K = w.shape[0], w.shape[1], 2
    else:
        Cout, Cin, K = w.shape[0], w.shape[1], w.shape[2]
    nbytes = lib.nps_conv3d_packed_bytes(Cout, Cin, K, 1 if transposed else 0, 1 if bf16 else 0)
    out = torch.empty(nbytes // (2 if bf16 else 4), dtype=torch.bfloat16 if bf16 else torch.float32, device=w.device)
    check(lib.nps_conv3d_pack_weights(ptr(w), ptr(out), Cout, Cin, K, 1 if transposed else 0, 1 if bf16 else 0,
                                      stream_ptr()), "conv3d_pack_weights")
    return out


def gn_stats3d(srcs: Sequence[Src3], frame_dhw, groups: int) -> torch.Tensor:
    """(B, groups, 2) fp64 (sum, sum of squares) of the virtual NDHWC frame's GroupNorm groups."""
    a = _fill_frame3(Conv3dArgs(), srcs, frame_dhw)
    st = torch.zeros((a.B, groups, 2), dtype=torch.float64, device=srcs[0].t.device)
    check(lib.nps_gn_stats3d(ctypes_byref(a), groups, ptr(st), stream_ptr()), "gn_stats3d")
    return st


# 3-D GroupNorm(1) frames take their sources' carried moments (the 3-D convs' out_stats) instead of an nps_gn_stats3d
# pass over the frame (dev knob NPS_CARRY3D=0: always the pass)
CARRY3D = os.environ.get("NPS_CARRY3D", "1") != "0"


def source_stats3d(t: torch.Tensor) -> torch.Tensor:
    """NDHWC t's GroupNorm(1) moments: carried, or one nps_gn_stats3d pass (then carried)."""
    st = stats_of(t)
    if st is None:
        st = gn_stats3d([Src3(t)], tuple(t.shape[1:4]), 1)
        attach_stats(t, st)
    return st


def group_norm_stats3d(srcs: Sequence[Src3], frame_dhw, groups: int) -> torch.Tensor:
    """gn_stats3d of a 3-D frame; GroupNorm(1) of sources that lie wholly inside the frame (crop_Nd zero-pads them,
    it does not cut them): the sum of the sources' carried moments (source_stats3d), as the 2-D group_norm_stats."""
    t0 = srcs[0].t
    if CARRY3D and groups == 1 and all(
            all(0 <= o and o + n <= f for o, n, f in zip((s.off_d, s.off_h, s.off_w), s.t.shape[1:4], frame_dhw))
            for s in srcs):
        parts = [source_stats3d(s.t) for s in srcs]
        if len(parts) == 1 and parts[0].shape[1] == 1:
            return parts[0]
        return _stats_sum(parts, t0.shape[0], new_stats(t0.shape[0], t0, 1))
    return gn_stats3d(srcs, frame_dhw, groups)


# Materialise act(GN(frame)) before a K > 1 conv whose frame needs a prologue or several / offset / unaligned
# sources (nps_frame_pack3d), so the conv runs its single-source fast path (dev knob NPS_CONV3D_PACK=0: off)
CONV3D_PACK = os.environ.get("NPS_CONV3D_PACK", "1") == "1"


def frame_pack3d(srcs: Sequence[Src3], frame_dhw, gn: Optional[GN] = None, pre_act=0) -> torch.Tensor:
    """(B, Dc, Hc, Wc, Cpad) = act(GN(virtual frame)), channels zero-padded to a multiple of 16."""
    a = _fill_frame3(Conv3dArgs(), srcs, frame_dhw)
    _set_prologue(a, gn, pre_act)
    cpad = (a.Cin + 15) // 16 * 16
    out = torch.empty((a.B, a.Dc, a.Hc, a.Wc, cpad), dtype=srcs[0].t.dtype, device=srcs[0].t.device)
    check(lib.nps_frame_pack3d(ctypes_byref(a), ptr(out), cpad, stream_ptr()), "frame_pack3d")
    return out


def _fp32_frame3(a, what):
    if a.bf16:
        raise NotImplementedError(f"nps_hip {what}: fp32 only (the 3-D frames differentiate fp32 tensors; use fp32 "
                                  "for training)")


def frame3d(srcs: Sequence[Src3], frame_dhw, gn: Optional[GN] = None, pre_act=0) -> torch.Tensor:
    """(B, Dc, Hc, Wc, Cin) fp32 = act(GN(virtual frame)) with exactly Cin channels (nps_frame3d_fwd): the frame of
    the differentiable 3-D walk (the conv weight's own Cin, no channel padding, erf GELU).  Without gn and pre_act
    this is crop_Nd in 3-D."""
    a = _fill_frame3(Conv3dArgs(), srcs, frame_dhw)
    _fp32_frame3(a, "frame3d")
    _set_prologue(a, gn, pre_act)
    out = torch.empty((a.B, a.Dc, a.Hc, a.Wc, a.Cin), dtype=torch.float32, device=srcs[0].t.device)
    check(lib.nps_frame3d_fwd(ctypes_byref(a), ptr(out), stream_ptr()), "frame3d_fwd")
    return out


def frame3d_bwd(srcs: Sequence[Src3], frame_dhw, gn: Optional[GN], pre_act, gy: torch.Tensor,
                gy_plain: Optional[torch.Tensor] = None, need: Optional[Sequence[bool]] = None):
    """The backward of frame3d (nps_frame3d_bwd): (dsrc list, dgamma, dbeta) given gy = dL/d(frame) and gy_plain
    (or None), the gradient of the plain concatenation of the same sources.  need[i] False: source i gets no
    gradient (None).  dgamma / dbeta are None without a GroupNorm."""
    a = _fill_frame3(Conv3dArgs(), srcs, frame_dhw)
    _fp32_frame3(a, "frame3d_bwd")
    _set_prologue(a, gn, pre_act)
    shape = (a.B, a.Dc, a.Hc, a.Wc, a.Cin)
    for g in (gy, gy_plain):
        if g is not None and (tuple(g.shape) != shape or g.dtype != torch.float32 or not g.is_contiguous()):
            raise RuntimeError(f"nps_hip frame3d_bwd: gradients must be contiguous fp32 {shape}, got {tuple(g.shape)}")
    dgamma = dbeta = work = None
    if gn is not None:
        dgamma, dbeta = torch.empty_like(gn.gamma), torch.empty_like(gn.beta)
        work = new_stats(a.B, gy, a.Cin)  # zero on entry: a slice of a zeroed chunk
    need = [True] * len(srcs) if need is None else need
    dsrc = [torch.empty_like(s.t) if need[i] else None for i, s in enumerate(srcs)]
    arr = (ctypes.c_void_p * 3)(*[ptr(d) for d in dsrc] + [None] * (3 - len(dsrc)))
    check(lib.nps_frame3d_bwd(ctypes_byref(a), ptr(gy), ptr(gy_plain), arr, ptr(dgamma), ptr(dbeta), ptr(work),
                              stream_ptr()), "frame3d_bwd")
    return dsrc, dgamma, dbeta


def add_at_copy3d(base: torch.Tensor, src: torch.Tensor, off=(0, 0, 0)) -> torch.Tensor:
    """base + crop_Nd(src) placed at `off` (per axis: > 0 zero-pads, < 0 crops), NDHWC fp32, one pass."""
    for t in (base, src):
        if t.dtype != torch.float32 or t.dim() != 5 or not t.is_contiguous():
            raise RuntimeError(f"nps_hip add_at_copy3d: contiguous fp32 NDHWC tensors, got {t.dtype} {tuple(t.shape)}")
    if base.shape[0] != src.shape[0] or base.shape[4] != src.shape[4]:
        raise RuntimeError("nps_hip add_at_copy3d: base and src must share batch and channels")
    B, Do, Ho, Wo, C = base.shape
    out = torch.empty_like(base)
    check(lib.nps_add_at_copy3d(ptr(out), ptr(base), ptr(src), B, Do, Ho, Wo, src.shape[1], src.shape[2],
                                src.shape[3], C, int(off[0]), int(off[1]), int(off[2]), stream_ptr()),
          "add_at_copy3d")
    return out


def conv3d(srcs: Sequence[Src3], frame_dhw, wpack: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, K: int,
           stride=1, transposed=False, circ=0, zpad=0, gn: Optional[GN] = None, pre_act=0,
           out: Optional[torch.Tensor] = None, out_os=1, out_off=(0, 0, 0), accumulate=False,
           addend: Optional[torch.Tensor] = None, act=0, out_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One nps_conv3d launch over a virtual NDHWC frame (sources at crop offsets), extended per side by
    `circ` circular then `zpad` zero voxels; valid K^3 conv (stride), or with `transposed` the 8 phase convs
    (K = 2) of a k4/s2 transposed conv written with out_os = 2.  Without `out` a tensor of the conv's
    output extent (x2 per axis when transposed) is allocated.  Returns `out`."""
    simple = (len(srcs) == 1 and gn is None and not pre_act and tuple(srcs[0].t.shape[1:4]) == tuple(frame_dhw)
              and not (srcs[0].off_d or srcs[0].off_h or srcs[0].off_w) and srcs[0].t.shape[4] % 16 == 0)
    cin_alg = sum(s.t.shape[4] for s in srcs)  # algorithmic input channels (before channel padding)
    if CONV3D_PACK and K > 1 and not simple:
        srcs, gn, pre_act = [Src3(frame_pack3d(srcs, frame_dhw, gn, pre_act))], None, 0
    a = _fill_frame3(Conv3dArgs(), srcs, frame_dhw)
    ext = 2 * (circ + zpad)
    Dout, Hout, Wout = ((n + ext - K) // stride + 1 for n in (a.Dc, a.Hc, a.Wc))
    if min(Dout, Hout, Wout) <= 0:
        raise RuntimeError(f"nps_hip conv3d: empty output for frame {tuple(frame_dhw)} K={K}")
    dt = srcs[0].t.dtype
    if (wpack.dtype == torch.bfloat16) != (dt == torch.bfloat16):
        raise RuntimeError("nps_hip conv3d: weight packing dtype must match the activations")
    if out is None:
        f = 2 if transposed else 1
        out = torch.empty((a.B, f * Dout, f * Hout, f * Wout, Cout), dtype=dt, device=srcs[0].t.device)
        if transposed:
            out_os = 2
    if out.dtype != dt or not out.is_contiguous() or out.dim() != 5:
        raise RuntimeError("nps_hip conv3d: out must be contiguous NDHWC of the sources' dtype")
    if addend is not None and (addend.shape != out.shape or addend.dtype != dt or not addend.is_contiguous()):
        raise RuntimeError("nps_hip conv3d: addend must be laid out like out")
    a.circ, a.zpad = circ, zpad
    _set_prologue(a, gn, pre_act)
    a.K, a.stride, a.transposed = K, stride, 1 if transposed else 0
    a.Dout, a.Hout, a.Wout = Dout, Hout, Wout
    a.out_stats = ptr(out_stats)  # (new_stats(B, ..) buffer: the stored values' GroupNorm(1) moments)
    a.wpack, a.bias, a.Cout = ptr(wpack), ptr(bias), Cout
    a.out, a.out_C, a.out_D, a.out_H, a.out_W = ptr(out), out.shape[4], out.shape[1], out.shape[2], out.shape[3]
    a.out_os, (a.out_off_d, a.out_off_h, a.out_off_w) = out_os, out_off
    a.accumulate, a.addend, a.act = 1 if accumulate else 0, ptr(addend), act
    if conv_probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.nps_conv3d_fwd(ctypes_byref(a), stream_ptr()), "conv3d")
        e1.record()
        nph = 8 if transposed else 1
        es = 2 if a.bf16 else 4
        nbytes = es * (sum(s.t.numel() for s in srcs) + nph * Cout * cin_alg * K ** 3 + nph * a.B * Dout * Hout * Wout * Cout)
        conv_probe.append((e0, e1, 2.0 * nph * a.B * Dout * Hout * Wout * Cout * cin_alg * K ** 3,
                           ("bf16_3d" if a.bf16 else "f32_3d", K ** 3, 4), nbytes))
    else:
        check(lib.nps_conv3d_fwd(ctypes_byref(a), stream_ptr()), "conv3d")
    return out


# ---- 3-D conv backward: weight derivations (torch ops on the parameter, any device), weight gradient, layout helpers
def conv3d_dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv3d weight (Cout, Cin, K, K, K) -> the stride-1 input gradient's conv weight (Cin, Cout, K, K, K): all
    three taps flipped, channels swapped.  dx = conv3d(dy extended by K - 1 - p per side, this) for a conv padded
    by p (zeros), or the circular conv of dy for circular 'same' padding."""
    return w.detach().flip(2, 3, 4).transpose(0, 1).contiguous()


def conv3d_s2_dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) of a stride-2 conv -> the (Cout, Cin, 4, 4, 4) nn.ConvTranspose3d
    weight whose k4/s2 transposed conv of dy is the input gradient (shifted by the conv's padding): the adjoint is
    a k3/s2 transposed conv, i.e. a k4/s2 one whose fourth tap per axis is zero."""
    return torch.nn.functional.pad(w.detach(), (0, 1, 0, 1, 0, 1)).contiguous()


def conv_transpose3d_dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.ConvTranspose3d weight (Cin, Cout, 4, 4, 4) of a k4/s2 transposed conv -> the (Cin, 8 Cout, 2, 2, 2) conv
    weight of its input gradient over the space-to-depth of dy (space_to_depth3d): channel ((rd*2 + rh)*2 + rw)*Cout
    + co, tap (td, th, tw) holds w[ci, co, 2 td + rd, 2 th + rh, 2 tw + rw]."""
    Cin, Cout = w.shape[:2]
    return (w.detach().reshape(Cin, Cout, 2, 2, 2, 2, 2, 2).permute(0, 3, 5, 7, 1, 2, 4, 6)
            .reshape(Cin, 8 * Cout, 2, 2, 2).contiguous())


def _wgrad3d_args(a: torch.Tensor, x: torch.Tensor, K: int, stride: int, circ: int, zpad: int) -> Wgrad3dArgs:
    for t in (a, x):
        if t.dtype != torch.float32 or t.dim() != 5 or not t.is_contiguous():
            raise RuntimeError(f"nps_hip conv3d_wgrad: contiguous fp32 NDHWC tensors, got {t.dtype} {tuple(t.shape)}")
    if a.shape[0] != x.shape[0]:
        raise RuntimeError("nps_hip conv3d_wgrad: a and x must share the batch")
    p = Wgrad3dArgs()
    p.a, (p.B, p.Da, p.Ha, p.Wa, p.M) = ptr(a), a.shape
    p.x, (_, p.Dx, p.Hx, p.Wx, p.N) = ptr(x), x.shape
    p.K, p.stride, p.circ, p.zpad = K, stride, circ, zpad
    return p


def conv3d_wgrad_splits(a: torch.Tensor, x: torch.Tensor, K: int, stride=1, circ=0, zpad=0) -> int:
    """How many work-groups share each (m tile, n tile, tap group)'s voxel reduction in conv3d_wgrad's launch."""
    p = _wgrad3d_args(a, x, K, stride, circ, zpad)
    p.g = p.a  # (the plan only needs a non-NULL pointer)
    n = lib.nps_conv3d_wgrad_splits(ctypes_byref(p))
    check(0 if n > 0 else n, "conv3d_wgrad_splits")
    return n


def conv3d_wgrad(a: torch.Tensor, x: torch.Tensor, K: int, stride=1, circ=0, zpad=0,
                 g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g[M][N][K][K][K] (+)= sum over a's voxels p of a[p][m] * Xext[p*stride + tap][n] (nps_conv3d_wgrad, exact fp32
    MFMA): x (B, Dx, Hx, Wx, N) extended per side by `circ` circular then `zpad` zero voxels, a (B, Da, Ha, Wa, M) of
    the valid K^3 / stride conv's output extent.  Without g a zero-filled one is allocated; a given g is added to."""
    p = _wgrad3d_args(a, x, K, stride, circ, zpad)
    if g is None:
        g = torch.zeros((p.M, p.N, K, K, K), dtype=torch.float32, device=a.device)
    elif g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != p.M * p.N * K ** 3:
        raise RuntimeError("nps_hip conv3d_wgrad: g must be contiguous fp32 [M][N][K][K][K]")
    p.g = ptr(g)
    check(lib.nps_conv3d_wgrad(ctypes_byref(p), stream_ptr()), "conv3d_wgrad")
    return g


def space_to_depth3d(x: torch.Tensor, Dq: int, Hq: int, Wq: int) -> torch.Tensor:
    """(B, D, H, W, C) fp32 -> (B, Dq, Hq, Wq, 8 C): channel ((rd*2 + rh)*2 + rw)*C + c = x[2 dq + rd, 2 hq + rh,
    2 wq + rw, c] (0 outside x)."""
    B, D, H, W, C = x.shape
    out = torch.empty((B, Dq, Hq, Wq, 8 * C), dtype=torch.float32, device=x.device)
    check(lib.nps_space_to_depth3d(ptr(x), ptr(out), B, D, H, W, C, Dq, Hq, Wq, stream_ptr()), "space_to_depth3d")
    return out


def circular_pad3d(x: torch.Tensor, pad: int) -> torch.Tensor:
    """(B, D, H, W, C) fp32 -> circularly padded by `pad` voxels per side of every axis."""
    B, D, H, W, C = x.shape
    out = torch.empty((B, D + 2 * pad, H + 2 * pad, W + 2 * pad, C), dtype=torch.float32, device=x.device)
    check(lib.nps_circular_pad3d(ptr(x), ptr(out), B, D, H, W, C, pad, stream_ptr()), "circular_pad3d")
    return out


def circular_fold3d(gp: torch.Tensor, pad: int) -> torch.Tensor:
    """The adjoint of circular_pad3d: (B, D + 2 pad, H + 2 pad, W + 2 pad, C) -> the wrap-sum (B, D, H, W, C)."""
    B, Dp, Hp, Wp, C = gp.shape
    D, H, W = Dp - 2 * pad, Hp - 2 * pad, Wp - 2 * pad
    out = torch.empty((B, D, H, W, C), dtype=torch.float32, device=gp.device)
    check(lib.nps_circular_fold3d(ptr(gp), ptr(out), B, D, H, W, C, pad, stream_ptr()), "circular_fold3d")
    return out


# ------------------------------------------------------------ 1-D U-Net convs -----
class Src1(NamedTuple):
    t: torch.Tensor          # (B, L, C) channels-last contiguous fp32
    off: int = 0             # placement along L inside the frame (crop_Nd: > 0 zero-pads, < 0 crops)


def drop_tag(t: torch.Tensor):
    """Forget t's range tag: a kernel that knows no tags wrote into t."""
    if getattr(t, "_nps_tag", None) is not None:
        t._nps_tag = None


def _check1d(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"nps_hip ops run on the MI355X only: {what} is on {t.device}")
    if t.dtype != torch.float32:
        raise NotImplementedError(f"nps_hip {what}: the 1-D convs run fp32 tensors only, got {t.dtype}")


def _src1(s) -> Src1:
    """An ops.Src1, or an ops.Src of a (B, 1, L, C) map (its off_x is the offset along L), as a Src1 of (B, L, C)."""
    t = s.t
    off = s.off if isinstance(s, Src1) else s.off_x
    if t.dim() == 4:
        if t.shape[1] != 1 or (not isinstance(s, Src1) and s.off_y):
            raise RuntimeError(f"nps_hip conv1d: a 4-D source must be a (B, 1, L, C) map at row 0, got {tuple(t.shape)}")
        t = t.view(t.shape[0], t.shape[2], t.shape[3])
    return Src1(t, int(off))


def pack_conv1d_weight(w: torch.Tensor) -> torch.Tensor:
    """A conv weight (Cout, Cin, K) -> the nps_conv1d packing [K][Cin padded to 16][Cout padded to 64] (zeros in the
    padding)."""
    _check1d(w, "pack_conv1d_weight weight")
    w = w.detach().contiguous()
    Cout, Cin, K = w.shape
    n = lib.nps_conv1d_packed_floats(Cout, Cin, K)
    if n == 0:
        raise RuntimeError(f"nps_hip pack_conv1d_weight: unsupported weight shape {tuple(w.shape)} (K in 1..4)")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.nps_conv1d_pack_weights(ptr(w), ptr(out), Cout, Cin, K, stream_ptr()), "conv1d_pack_weights")
    out.nps_conv1d = (Cout, Cin, K)
    return out


def conv1d(srcs, L: int, wpack: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, K: int, stride=1, pad=(0, 0),
           out: Optional[torch.Tensor] = None, out_os=1, out_off=0, accumulate=False,
           addend: Optional[torch.Tensor] = None, act=0) -> torch.Tensor:
    """One nps_conv1d_fwd launch over a virtual channels-last frame of L positions (sources Src1 / (B, 1, L, C) Src at
    their crop offsets, zero outside themselves and outside the frame): the K-tap conv with stride 1 or 2 and
    (left, right) zero padding `pad`; out[b][l*out_os + out_off] = act(conv + bias + addend) (+= with accumulate),
    rows outside out dropped.  Without `out` a (B, Lout, Cout) tensor is allocated.  Returns `out`."""
    ss = [_src1(s) for s in srcs]
    for s in ss:
        _check1d(s.t, "conv1d source")
        if not s.t.is_contiguous() or s.t.dim() != 3 or s.t.shape[0] != ss[0].t.shape[0]:
            raise RuntimeError(f"nps_hip conv1d: sources must be contiguous (B, L, C) of one batch, got {tuple(s.t.shape)}")
    Cin = sum(s.t.shape[2] for s in ss)
    if getattr(wpack, "nps_conv1d", None) != (Cout, Cin, K):
        raise RuntimeError(f"nps_hip conv1d: the packing holds {getattr(wpack, 'nps_conv1d', None)}, the launch needs "
                           f"(Cout, Cin, K) = {(Cout, Cin, K)}")
    B, L = ss[0].t.shape[0], int(L)
    pl, pr = (int(pad), int(pad)) if isinstance(pad, int) else (int(pad[0]), int(pad[1]))
    Lout = (L + pl + pr - K) // stride + 1
    if Lout <= 0:
        raise RuntimeError(f"nps_hip conv1d: empty output for a frame of {L} padded by {(pl, pr)}, K={K}")
    if out is None:
        out = torch.empty((B, Lout, Cout), dtype=torch.float32, device=ss[0].t.device)
    else:
        _check1d(out, "conv1d out")
        drop_stats(out)
        drop_tag(out)
    if not out.is_contiguous() or out.dim() != 3 or out.shape[0] != B or out.shape[2] < Cout:
        raise RuntimeError(f"nps_hip conv1d: out must be contiguous (B, L, >= Cout), got {tuple(out.shape)}")
    if addend is not None:
        _check1d(addend, "conv1d addend")
        if addend.shape != out.shape or not addend.is_contiguous():
            raise RuntimeError("nps_hip conv1d: addend must be laid out like out")
    if bias is not None:
        _check1d(bias, "conv1d bias")
        if bias.numel() != Cout or not bias.is_contiguous():
            raise RuntimeError(f"nps_hip conv1d: bias must hold Cout = {Cout} contiguous values, got {tuple(bias.shape)}")
    a = Conv1dArgs()
    a.nsrc = len(ss)
    for i, s in enumerate(ss):
        a.src[i].ptr, a.src[i].C, a.src[i].L, a.src[i].off = ptr(s.t), s.t.shape[2], s.t.shape[1], s.off
    a.B, a.Lc, a.Cin = B, L, Cin
    a.K, a.stride, a.pad_l, a.pad_r, a.Lout = K, stride, pl, pr, Lout
    a.wpack, a.bias, a.Cout = ptr(wpack), ptr(bias), Cout
    a.out, a.out_C, a.out_L, a.out_os, a.out_off = ptr(out), out.shape[2], out.shape[1], out_os, int(out_off)
    a.accumulate, a.addend, a.act = 1 if accumulate else 0, ptr(addend), act
    if conv_probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.nps_conv1d_fwd(ctypes_byref(a), stream_ptr()), "conv1d_fwd")
        e1.record()
        nbytes = 4.0 * (sum(s.t.numel() for s in ss) + Cout * Cin * K + B * Lout * Cout)
        conv_probe.append((e0, e1, 2.0 * B * Lout * Cout * Cin * K, ("f32_1d", K, 4), nbytes))
    else:
        check(lib.nps_conv1d_fwd(ctypes_byref(a), stream_ptr()), "conv1d_fwd")
    return out


# ---- 1-D conv backward: the derived weights of the input gradients (torch ops on the parameter) and the weight gradient
def conv1d_dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv1d weight (Cout, Cin, K) -> the stride-1 input gradient's conv weight (Cin, Cout, K): taps flipped,
    channels swapped.  dx = conv1d(dy, this) padded by (K - 1 - pad_l, K - 1 - pad_r)."""
    return w.detach().flip(2).transpose(0, 1).contiguous()


def conv_transpose1d_phase_weights(w: torch.Tensor) -> List[torch.Tensor]:
    """nn.ConvTranspose1d weight (Cin, Cout, k <= 4) of a stride-2 transposed conv -> its two phases' 2-tap conv
    weights (Cout, Cin, 2): output 2 q + r - padding = sum_t W_r[:, :, t] x[q + t - 1], W_r[co, ci, t] =
    w[ci, co, 2 (1 - t) + r] (taps past k are zero)."""
    w = w.detach()
    if w.shape[2] < 4:
        w = torch.nn.functional.pad(w, (0, 4 - w.shape[2]))
    wt = w.transpose(0, 1)
    return [torch.stack((wt[:, :, 2 + r], wt[:, :, r]), dim=2).contiguous() for r in (0, 1)]


def _wgrad1d_args(a: torch.Tensor, x: torch.Tensor, K: int, stride: int, pad) -> Wgrad1dArgs:
    for t in (a, x):
        _check1d(t, "conv1d_wgrad tensor")
        if t.dim() != 3 or not t.is_contiguous():
            raise RuntimeError(f"nps_hip conv1d_wgrad: contiguous (B, L, C) tensors, got {tuple(t.shape)}")
    if a.shape[0] != x.shape[0]:
        raise RuntimeError("nps_hip conv1d_wgrad: a and x must share the batch")
    p = Wgrad1dArgs()
    p.a, (p.B, p.La, p.M) = ptr(a), a.shape
    p.x, (_, p.Lx, p.N) = ptr(x), x.shape
    p.K, p.stride = K, stride
    p.pad_l, p.pad_r = (int(pad), int(pad)) if isinstance(pad, int) else (int(pad[0]), int(pad[1]))
    return p


def conv1d_wgrad(a: torch.Tensor, x: torch.Tensor, K: int, stride=1, pad=(0, 0)) -> torch.Tensor:
    """g[M][N][K] = sum over a's positions of a[b][l][m] * xz[b][l*stride + t - pad_l][n] (nps_conv1d_wgrad, exact fp32
    MFMA, fixed split schedule + reduce pass: run twice, the bits are the same): x (B, Lx, N) zero-extended, a
    (B, La, M) of the K-tap / stride conv's output length over x padded by `pad`."""
    p = _wgrad1d_args(a, x, K, stride, pad)
    n = lib.nps_conv1d_wgrad_ws_floats(ctypes_byref(p))
    if n == 0:
        raise RuntimeError("conv1d_wgrad failed: " + lib.nps_last_error().decode())
    ws = torch.empty(n, dtype=torch.float32, device=a.device)
    g = torch.empty((p.M, p.N, K), dtype=torch.float32, device=a.device)
    p.g, p.ws = ptr(g), ptr(ws)
    check(lib.nps_conv1d_wgrad(ctypes_byref(p), stream_ptr()), "conv1d_wgrad")
    return g


# ------------------------------------------------------------------ data path -----
def gather_windows(u: torch.Tensor, steps, tw: int, offset: int) -> torch.Tensor:
    """out[b] = u[b][:, steps[b] + offset : steps[b] + offset + tw] for a device-resident trajectory batch
    u (B, C, T, *spatial) — DataCreator.create_data's per-sample windows (common/data_creator.py:48-78) as
    one HIP gather (nps_gather_windows)."""
    u = u.contiguous()
    B, C, T = u.shape[:3]
    HW = math.prod(u.shape[3:]) if u.dim() > 3 else 1
    if len(steps) != B:
        raise ValueError(f"gather_windows: {len(steps)} steps for a batch of {B}")
    for st in steps:
        if st + offset < 0 or st + offset + tw > T:
            raise AssertionError("this step - time window combination is not valid")
    st_dev = torch.tensor([int(v) for v in steps], dtype=torch.int32).to(u.device, non_blocking=True)
    out = torch.empty((B, C, tw) + tuple(u.shape[3:]), dtype=torch.float32, device=u.device)
    check(lib.nps_gather_windows(ptr(u), ptr(st_dev), ptr(out), B, C, T, HW, tw, offset, stream_ptr()),
          "gather_windows")
    return out


# ----------------------------------------------------------- misc kernels -----
def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    check(lib.nps_nchw_to_nhwc(ptr(x), ptr(out), B, C, H, W, stream_ptr()), "nchw_to_nhwc")
    return share_tag(out, x)


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    B, H, W, C = x.shape
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    check(lib.nps_nhwc_to_nchw(ptr(x), ptr(out), B, C, H, W, stream_ptr()), "nhwc_to_nchw")
    return share_tag(out, x)


def grid_pixels(u: torch.Tensor) -> int:
    """N, the flat pixel count of a model tensor (B, c, tw, *spatial) on a 1-D, 2-D or 3-D grid."""
    if not 4 <= u.dim() <= 6:
        raise RuntimeError(f"nps_hip: (B, c, tw, *spatial) with 1 to 3 spatial axes, got {tuple(u.shape)}")
    return math.prod(u.shape[3:])


def pack_grid_input(u, pos, cond, sc, Cp):
    """u (B, c, tw, *spatial) on a 1-D, 2-D or 3-D grid, pos (B, *spatial, P) with P = the grid's dimension (1-D: also
    (B, L)), cond (B, K) or None, sc (B, S, *spatial) or None -> (xin (B, N, Cp), vb (B, N, K+S) or None) over the
    N = prod(spatial) flat pixels; on a 2-D grid the (B, H, W, .) tensors."""
    N = grid_pixels(u)
    B, c, tw = u.shape[:3]
    spatial = tuple(u.shape[3:])
    if len(spatial) == 1 and pos.dim() == 2:
        pos = pos.unsqueeze(-1)  # enc_grid.py:43-44
    P = pos.shape[-1]
    if tuple(pos.shape) != (B,) + spatial + (P,):
        raise RuntimeError(f"pack_grid_input: pos {tuple(pos.shape)} does not lie on u's grid {spatial}")
    if sc is not None and tuple(sc.shape[2:]) != spatial:
        raise RuntimeError(f"pack_grid_input: spatial cond {tuple(sc.shape)} does not lie on u's grid {spatial}")
    K = 0 if cond is None else cond.shape[1]
    S = 0 if sc is None else sc.shape[1]
    shape = (B,) + spatial if len(spatial) == 2 else (B, N)
    xin = torch.empty(shape + (Cp,), dtype=torch.float32, device=u.device)
    vb = torch.empty(shape + (K + S,), dtype=torch.float32, device=u.device) if K + S > 0 else None
    check(lib.nps_pack_grid_input_nd(ptr(u), ptr(pos), ptr(cond), ptr(sc), ptr(xin), ptr(vb), B, c * tw, N, P, K, S,
                                     Cp, stream_ptr()), "pack_grid_input")
    return xin, vb


def timeconv_decode(pre, u, w1, b1, w2, b2, dtcum, mask, mask_ch, act_tanh, num_c, tw):
    """pre: the planar (B, 3*num_c*tw, N) pre-decoder output in any view; u, the model input (B, c, tw, *spatial) ->
    (B, num_c, tw, *spatial).  The chain is per pixel: the kernels take the flat pixel count as H * W."""
    B, N = u.shape[0], grid_pixels(u)
    out = torch.empty((B, num_c, tw) + tuple(u.shape[3:]), dtype=torch.float32, device=u.device)
    S = 0 if mask is None else mask.shape[1]
    check(lib.nps_timeconv_decode(ptr(pre), ptr(u), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dtcum), ptr(mask), S,
                                  mask_ch, ptr(out), B, num_c, tw, 1, N, 1 if act_tanh else 0, stream_ptr()),
          "timeconv_decode")
    return out


# the grid decoders' per-pixel chain (include/nps.h nps_decode_t)
DECODE_ACT_NONE, DECODE_ACT_GELU, DECODE_ACT_SWISH = 0, 1, 2
DELTA_MODES = {"per_step": 0, "all": 1, "none": 2}  # dec_grid.py:11


class DecodeSpec(NamedTuple):
    """The constants of one decode chain: the layout of its input (planar (B, C0*L0, N) or channels-last
    (B, N, C0*L0), in any view), stage 1's stride and activation, and the epilogue."""
    planar: bool
    C0: int
    L0: int
    num_c: int
    tw: int
    delta_mode: int = 0     # DELTA_MODES
    dt: float = 1.0         # 'all'
    s1: int = 1
    act: int = 0            # DECODE_ACT_*
    beta: float = 1.0       # Swish
    act_tanh: bool = False
    mask_ch: int = 0


def decode_args(spec: DecodeSpec, x, u, w1, b1, w2, b2, dtcum, mask, out=None) -> DecodeArgs:
    """nps_decode_t of a chain on x with the stages that have weights (w1 (C1, C0, k1) or None, w2 (C2, C1, k2) or
    None); u is the model input (B, num_c, tw, *spatial)."""
    B, N = u.shape[0], grid_pixels(u)
    CL = spec.C0 * spec.L0
    if x.numel() != B * N * CL or not x.is_contiguous() or x.dtype != torch.float32:
        raise RuntimeError(f"decode_chain: x {tuple(x.shape)} is not a contiguous fp32 tensor of B={B} x N={N} pixels "
                           f"x C0*L0={spec.C0}*{spec.L0}")
    if w2 is not None and w1 is None:
        raise RuntimeError("decode_chain: a second stage needs a first")
    d = DecodeArgs()
    d.x = ptr(x)
    d.x_bs, d.x_ps, d.x_cs = (CL * N, 1, N) if spec.planar else (N * CL, CL, 1)
    d.B, d.N, d.C0, d.L0 = B, N, spec.C0, spec.L0
    d.nstage = (w1 is not None) + (w2 is not None)
    if w1 is not None:
        d.C1, d.k1, d.s1, d.act, d.beta = w1.shape[0], w1.shape[2], spec.s1, spec.act, float(spec.beta)
        d.w1, d.b1 = ptr(w1), ptr(b1)
    if w2 is not None:
        d.C2, d.k2 = w2.shape[0], w2.shape[2]
        d.w2, d.b2 = ptr(w2), ptr(b2)
    d.u, d.num_c, d.tw = ptr(u), spec.num_c, spec.tw
    d.delta_mode, d.dt, d.dtcum = spec.delta_mode, float(spec.dt), ptr(dtcum)
    d.act_tanh = 1 if spec.act_tanh else 0
    if mask is not None:
        d.mask, d.mask_S, d.mask_ch = ptr(mask), mask.shape[1], spec.mask_ch
    d.out = ptr(out)
    return d


def decode_chain(spec: DecodeSpec, x, u, w1=None, b1=None, w2=None, b2=None, dtcum=None, mask=None):
    """The decoders' per-pixel chain on HIP (nps_decode_fwd): up to two Conv1d stages over each pixel's signal in x,
    add_delta in the mode of spec, tanh and the spatial-cond mask -> (B, num_c, tw, *spatial)."""
    out = torch.empty((u.shape[0], spec.num_c, spec.tw) + tuple(u.shape[3:]), dtype=torch.float32, device=u.device)
    d = decode_args(spec, x, u, w1, b1, w2, b2, dtcum, mask, out)
    check(lib.nps_decode_fwd(ctypes.byref(d), stream_ptr()), "decode_chain")
    return out


def plane_sums(base: torch.Tensor, offset: int, plane_stride: int, plane_size: int, nplanes: int) -> torch.Tensor:
    sums = torch.empty(nplanes, dtype=torch.float64, device=base.device)
    check(lib.nps_plane_sums(ptr(base) + 4 * offset, plane_stride, plane_size, nplanes, ptr(sums), stream_ptr()),
          "plane_sums")
    return sums


def volume_rescale(u, new_tot, prev_tot, mpdcum, mask, mask_ch):
    B, c, tw, H, W = u.shape
    S = 0 if mask is None else mask.shape[1]
    check(lib.nps_volume_rescale(ptr(u), ptr(new_tot), ptr(prev_tot), ptr(mpdcum), ptr(mask), S, mask_ch, B, c, tw,
                                 H, W, stream_ptr()), "volume_rescale")
    return u


VOLUME_MODES = {"block": 0, "individual": 1}  # NPS_VOLUME_* of include/nps.h


def volume_factors(new_tot, prev_tot, mode: str, max_pct_dif: float, B: int, c: int, tw: int) -> torch.Tensor:
    """F (B, c, tw) of approx_volume_preserve_mode 'block' / 'individual' (activation_wrapper.py:40-79) from the fp64
    plane totals of u and of the input's last time step; the scalars stay fp64 on the device."""
    F = torch.empty(B, c, tw, dtype=torch.float32, device=new_tot.device)
    check(lib.nps_volume_factors(ptr(new_tot), ptr(prev_tot), VOLUME_MODES[mode], float(max_pct_dif), ptr(F), B, c,
                                 tw, stream_ptr()), "volume_factors")
    return F


def volume_apply(u, F, mask, mask_ch):
    """In place: u[b, c, t] *= F[b, c, t], then the spatial-cond mask re-applied (activation_wrapper.py:104-105)."""
    B, c, tw, H, W = u.shape
    S = 0 if mask is None else mask.shape[1]
    check(lib.nps_volume_apply(ptr(u), ptr(F), ptr(mask), S, mask_ch, B, c, tw, H, W, stream_ptr()), "volume_apply")
    return u


def sq_err_sum(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    a = a.contiguous()
    b = b.contiguous()
    if a.shape != b.shape:
        raise RuntimeError(f"sq_err_sum: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(lib.nps_sq_err_sum(ptr(a), ptr(b), a.numel(), ptr(out), stream_ptr()), "sq_err_sum")
    return out[0]


# -------------------------------------------------------------- U-Net self-attention ----
def _attn_check(qkv: torch.Tensor, heads: int, dk: int):
    if not qkv.is_cuda:
        raise RuntimeError("nps_hip ops run on the MI355X only: tensor is on " + str(qkv.device))
    if qkv.dtype != torch.float32 or not qkv.is_contiguous() or qkv.dim() != 3 or qkv.shape[2] != heads * 3 * dk:
        raise RuntimeError(f"attention: qkv must be contiguous fp32 (B, N, heads * 3 * dk), got {qkv.dtype} "
                           f"{tuple(qkv.shape)} for heads={heads}, dk={dk}")


def attention(qkv: torch.Tensor, heads: int, dk: int, scale: float):
    """proc_unet_modern.py:300-308 on the projection's output qkv (B, N, heads * 3 * dk), per head [q | k | v]:
    softmax over the QUERY index for each key (dim=1), never materialising the scores.  Returns
    (out (B, N, heads * dk), lse (B, heads, N)) — lse is what attention_bwd recomputes the weights from."""
    _attn_check(qkv, heads, dk)
    B, N = qkv.shape[0], qkv.shape[1]
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    out = torch.empty((B, N, heads * dk), dtype=torch.float32, device=qkv.device)
    check(lib.nps_attn_colstats(ptr(qkv), ptr(lse), B, N, heads, dk, float(scale), stream_ptr()), "attn_colstats")
    check(lib.nps_attn_fwd(ptr(qkv), ptr(lse), ptr(out), B, N, heads, dk, float(scale), stream_ptr()), "attn_fwd")
    return out, lse


def attention_bwd(qkv: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, heads: int, dk: int, scale: float):
    """Gradient of attention() with respect to qkv (same layout)."""
    _attn_check(qkv, heads, dk)
    B, N = qkv.shape[0], qkv.shape[1]
    dout = dout.contiguous()
    if dout.dtype != torch.float32 or tuple(dout.shape) != (B, N, heads * dk) or tuple(lse.shape) != (B, heads, N):
        raise RuntimeError("attention_bwd: dout must be fp32 (B, N, heads * dk) and lse (B, heads, N)")
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(lib.nps_attn_bwd_ws_floats(B, N, heads, dk), dtype=torch.float32, device=qkv.device)
    check(lib.nps_attn_bwd(ptr(qkv), ptr(lse), ptr(dout), ptr(dqkv), ptr(ws), B, N, heads, dk, float(scale),
                           stream_ptr()), "attn_bwd")
    return dqkv
