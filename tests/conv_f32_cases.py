"""Shared pieces of the exact-fp32 conv tests (NPS_CONV_PRECISION=f32): the precision switch, the host planner call,
the forward / weight-gradient case tables with the kernel instantiation each row is meant to reach, their fp64 / fp32
CPU references and the GPU drivers.  No tests here: tests/test_conv_f32_host.py (no GPU) and
tests/test_gpu_conv_f32.py use it.

Under PREC_F32 nps_conv2d_fwd launches (csrc/conv2d.hip)
  conv2d_pc_kernel<NTAPS, CKB, PB, CBW, WCO>  stride-1 undilated 1x1 / 2x2 / 3x3 without prologue (planned waves = 8):
      <1,32,2,3,2> 1x1, 8x16 tile, 192 channels per work-group, 32-channel stages
      <9,16,2,2,1> / <4,16,2,2,1>  3x3 / 2x2, 256-pixel tiles (16x16, 8x32), 64 channels, 16-channel stages
      <9,16,1,2,1> / <4,16,1,2,1>  3x3 / 2x2, 128-pixel 8x16 tile
  conv2d_fwd_kernel<WAVES>  everything else (5x5, dilation, stride 2, fused GroupNorm / GELU prologue): <4> 16x16 and
      8x32, <2> 8x16, <1> 8x8 and 4x16
and ad.wgrad launches wgrad_kernel (csrc/backward.hip) for every weight gradient."""
import contextlib
import ctypes
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

DEV = "cuda"
TOL = 1e-5          # the project's parity bar (tests/test_gpu_parity.py, BASELINE.json)
GN_EPS = 1e-5

PC = {(1, 128): "conv2d_pc_kernel<1,32,2,3,2>",
      (9, 256): "conv2d_pc_kernel<9,16,2,2,1>", (9, 128): "conv2d_pc_kernel<9,16,1,2,1>",
      (4, 256): "conv2d_pc_kernel<4,16,2,2,1>", (4, 128): "conv2d_pc_kernel<4,16,1,2,1>"}
ALL_INSTANTIATIONS = sorted(list(PC.values()) + [f"conv2d_fwd_kernel<{w}>" for w in (1, 2, 4)])
# every (waves, TH, TW) an exact-fp32 launch can carry
ALL_TILES = {(8, 16, 16), (8, 8, 32), (8, 8, 16), (4, 16, 16), (4, 8, 32), (2, 8, 16), (1, 8, 8), (1, 4, 16)}


@contextlib.contextmanager
def f32_precision():
    """ops.CONV_PRECISION = PREC_F32 inside the block (every reader takes it at call time; the pack cache keys on it)."""
    from nps_hip import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = ops.PREC_F32
    try:
        yield
    finally:
        ops.CONV_PRECISION = old


def out_size(n, k, stride=1, dil=1, pad=0, pad_hi=None, circ=0):
    pad_hi = pad if pad_hi is None else pad_hi
    return (n + 2 * circ + pad + pad_hi - dil * (k - 1) - 1) // stride + 1


def plan_f32(B, Cin, Cout, k, H, W, stride=1, dil=1, pad=(0, 0), pad_bottom=None, circ=0, gn=False, pre_act=0,
             out_nchw=0, srcs=None) -> Tuple[int, int, int]:
    """(waves, TH, TW) nps_conv2d_plan picks under NPS_PREC_F32 for this geometry (host arithmetic only; H x W is the
    unpadded frame, srcs an optional list of per-source channel counts)."""
    import nps_hip
    from nps_hip import ops
    pb = pad if pad_bottom is None else pad_bottom
    a = nps_hip.Conv2dArgs()
    cs = list(srcs) if srcs else [Cin]
    a.nsrc = len(cs)
    for i, c in enumerate(cs):
        a.src[i].ptr, a.src[i].C, a.src[i].H, a.src[i].W = 0x1000 * (i + 1), c, H, W
    a.B, a.Hin, a.Win, a.Cin = B, H, W, Cin
    a.KH = a.KW = k
    a.stride, a.dil, a.pad_y, a.pad_x, a.circ = stride, dil, pad[0], pad[1], circ
    a.Hout = out_size(H, k, stride, dil, pad[0], pb[0], circ)
    a.Wout = out_size(W, k, stride, dil, pad[1], pb[1], circ)
    a.Cout, a.out_C, a.out_H, a.out_W, a.out_os = Cout, Cout, a.Hout, a.Wout, 1
    a.out_nchw = out_nchw
    a.precision = ops.PREC_F32
    if gn:
        a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_groups, a.gn_eps = 0x8000, 0x9000, 0xa000, int(gn), GN_EPS
    a.pre_act = pre_act
    if nps_hip.lib.nps_conv2d_plan(ctypes.byref(a)) < 0:
        raise RuntimeError("conv2d_plan: " + nps_hip.lib.nps_last_error().decode())
    return a.waves, a.TH, a.TW


class Case(NamedTuple):
    name: str
    plan: Tuple[int, int, int]      # (waves, TH, TW) the launch carries
    B: int
    srcs: tuple                     # ((C, H, W, off_y, off_x), ...) NHWC sources placed in the frame
    frame: Tuple[int, int]
    Cout: int
    k: int
    stride: int = 1
    dil: int = 1
    pad: Tuple[int, int] = (0, 0)
    pad_bottom: Optional[Tuple[int, int]] = None
    circ: int = 0
    gn: int = 0                     # GroupNorm groups of the fused prologue (0: none)
    pre_act: int = 0
    bias: bool = True
    act: int = 0
    addends: int = 0
    add_after_act: bool = False
    accumulate: bool = False
    out_nchw: bool = False
    out_C: Optional[int] = None
    out_os: int = 1
    out_off: Tuple[int, int] = (0, 0)
    out_hw: Optional[Tuple[int, int]] = None   # size of `out` (default: out_os * conv output)
    forced: bool = False            # tile set by hand in a caller-filled nps_conv2d_t (the planner never picks it)

    @property
    def Cin(self):
        return sum(s[0] for s in self.srcs)

    @property
    def conv_hw(self):
        pb = self.pad if self.pad_bottom is None else self.pad_bottom
        return (out_size(self.frame[0], self.k, self.stride, self.dil, self.pad[0], pb[0], self.circ),
                out_size(self.frame[1], self.k, self.stride, self.dil, self.pad[1], pb[1], self.circ))

    @property
    def out_shape(self):
        """logical (B, out_C, out_H, out_W)"""
        Ho, Wo = self.conv_hw
        oh, ow = self.out_hw if self.out_hw is not None else (Ho * self.out_os, Wo * self.out_os)
        return self.B, self.out_C or self.Cout, oh, ow

    @property
    def kernel(self):
        """the instantiation the row is meant to reach"""
        w, th, tw = self.plan
        return PC[(self.k * self.k, th * tw)] if w == 8 else f"conv2d_fwd_kernel<{w}>"

    @property
    def stages(self):
        """K stages of the producer/consumer ring, as the kernel derives them: ceil(ceil(Cin / 16) / SUB)"""
        sub = 2 if self.k == 1 else 1
        return -(-(-(-self.Cin // 16)) // sub)

    def planned(self):
        return plan_f32(self.B, self.Cin, self.Cout, self.k, self.frame[0], self.frame[1], self.stride, self.dil,
                        self.pad, self.pad_bottom, self.circ, self.gn, self.pre_act, int(self.out_nchw),
                        [s[0] for s in self.srcs])


def _row(name, plan, B, cin, Cout, k, H, W, **kw):
    """cin: one source's channel count (covering the frame) or a tuple of sources (C, H, W, off_y, off_x)."""
    srcs = ((cin, H, W, 0, 0),) if isinstance(cin, int) else tuple(cin)
    return Case(name, plan, B, srcs, (H, W), Cout, k, **kw)


_CROP = ((20, 20, 20, 0, 0), (12, 17, 17, 1, 2), (4, 23, 23, -2, -1))  # crop_Nd offsets of both signs, uncovered pixels


def _epilogues(tag, plan, cin, Cout, k, H, W, **geo):
    Ho, Wo = out_size(H, k, pad=geo.get("pad", (0, 0))[0]), out_size(W, k, pad=geo.get("pad", (0, 0))[1])
    rows = [
        _row(f"{tag}_nobias", plan, 2, cin, Cout, k, H, W, bias=False, **geo),
        _row(f"{tag}_gelu", plan, 2, cin, Cout, k, H, W, act=1, **geo),
        _row(f"{tag}_addend", plan, 2, cin, Cout, k, H, W, addends=1, **geo),
        _row(f"{tag}_addend2_gelu", plan, 2, cin, Cout, k, H, W, addends=2, act=1, **geo),
        _row(f"{tag}_add_after_act", plan, 2, cin, Cout, k, H, W, addends=2, act=1, add_after_act=True, **geo),
        _row(f"{tag}_accumulate", plan, 2, cin, Cout, k, H, W, accumulate=True, addends=1, **geo),
        _row(f"{tag}_nchw", plan, 2, cin, Cout, k, H, W, out_nchw=True, act=1, addends=1, **geo),
        _row(f"{tag}_nchw_add_after_act", plan, 2, cin, Cout, k, H, W, out_nchw=True, act=1, addends=2,
             add_after_act=True, **geo),
        _row(f"{tag}_nchw_accumulate", plan, 2, cin, Cout, k, H, W, out_nchw=True, accumulate=True, **geo),
        _row(f"{tag}_wide_out", plan, 2, cin, Cout, k, H, W, out_C=Cout + 8, **geo),
        _row(f"{tag}_wide_out_odd", plan, 2, cin, Cout, k, H, W, out_C=Cout + 3, addends=1, **geo),
        # out_off -1 with a short `out`: the first and the last output row / column are dropped
        _row(f"{tag}_os2_crop", plan, 2, cin, Cout, k, H, W, out_os=2, out_off=(-1, -1),
             out_hw=(2 * Ho - 4, 2 * Wo - 4), **geo),
    ]
    rows += [_row(f"{tag}_os2_{py}{px}", plan, 2, cin, Cout, k, H, W, out_os=2, out_off=(py, px), act=py, **geo)
             for py in (0, 1) for px in (0, 1)]
    return rows


FORWARD_CASES = [
    # ---- one row per instantiation / tile shape (the smallest shapes that plan to them)
    _row("pc3x3_8x16", (8, 8, 16), 2, 16, 64, 3, 20, 20),
    _row("pc3x3_16x16", (8, 16, 16), 2, 20, 512, 3, 66, 66),
    _row("pc3x3_8x32", (8, 8, 32), 4, 4, 1024, 3, 10, 130),
    _row("pc2x2_8x16", (8, 8, 16), 2, 48, 40, 2, 17, 19),
    _row("pc2x2_16x16", (8, 16, 16), 2, 16, 512, 2, 65, 65),
    _row("pc2x2_8x32", (8, 8, 32), 4, 16, 1024, 2, 9, 129),
    _row("pc1x1", (8, 8, 16), 2, 20, 192, 1, 13, 11),
    _row("gen5x5_pad2", (4, 16, 16), 2, 12, 16, 5, 19, 21, pad=(2, 2)),
    _row("gen5x5_dil2_circ", (4, 8, 32), 2, 8, 8, 5, 24, 24, dil=2, circ=4),
    _row("gen3x3_s2", (2, 8, 16), 2, 2, 2, 3, 21, 22, stride=2),
    # conv2d_fwd_kernel<1>: the planner never returns waves = 1 (tests/test_conv_f32_host.py); nps_conv2d_fwd takes the
    # caller's tile with TH * TW == 64 * waves
    _row("gen1_8x8", (1, 8, 8), 2, 7, 5, 3, 11, 13, pad=(1, 1), forced=True),
    _row("gen1_4x16", (1, 4, 16), 2, 12, 20, 5, 9, 21, dil=2, circ=4, act=1, forced=True),
    _row("gen1_8x8_s2", (1, 8, 8), 2, 6, 70, 3, 19, 20, stride=2, addends=1, forced=True),
    # ---- stage count of the producer/consumer ring (1, 2, 3, 4, 5, 7), 4-channel tails, Cout tails
    _row("pc3x3_st2_co5", (8, 8, 16), 2, 20, 5, 3, 20, 22),
    _row("pc3x3_st3_co68", (8, 8, 16), 2, 36, 68, 3, 20, 22),
    _row("pc3x3_st4_co193", (8, 8, 16), 2, 52, 193, 3, 20, 22),
    _row("pc3x3_st5_co64", (8, 8, 16), 2, 68, 64, 3, 20, 22),
    _row("pc3x3_st7_co6", (8, 8, 16), 2, 100, 6, 3, 20, 22),
    _row("pc3x3_c7_fetch4", (8, 8, 16), 2, 7, 64, 3, 20, 22),
    _row("pc2x2_st1_co193", (8, 8, 16), 2, 16, 193, 2, 21, 20),
    _row("pc2x2_st2_co68", (8, 8, 16), 2, 20, 68, 2, 21, 20),
    _row("pc2x2_st3_co5", (8, 8, 16), 2, 36, 5, 2, 21, 20),
    _row("pc2x2_st4_co64", (8, 8, 16), 2, 52, 64, 2, 21, 20),
    _row("pc2x2_st5_co40", (8, 8, 16), 2, 68, 40, 2, 21, 20),
    _row("pc2x2_st7_co64", (8, 8, 16), 2, 100, 64, 2, 21, 20),
    _row("pc2x2_c7_fetch4", (8, 8, 16), 2, 7, 20, 2, 21, 20),
    _row("pc1x1_st2_co75", (8, 8, 16), 2, 36, 75, 1, 20, 21),
    _row("pc1x1_st3_co193", (8, 8, 16), 2, 68, 193, 1, 20, 21),
    _row("pc1x1_st4_co388", (8, 8, 16), 2, 100, 388, 1, 20, 21),
    _row("pc1x1_st5_co192", (8, 8, 16), 2, 132, 192, 1, 20, 21),
    _row("pc1x1_st7_co75", (8, 8, 16), 2, 196, 75, 1, 20, 21),
    _row("pc1x1_c7_fetch4", (8, 8, 16), 2, 7, 192, 1, 20, 21),
    # ---- padding, wrap, tile edges
    _row("pc3x3_pad1", (8, 8, 16), 2, 20, 40, 3, 20, 22, pad=(1, 1)),
    _row("pc3x3_circ1", (8, 8, 16), 2, 20, 40, 3, 20, 22, circ=1),
    _row("pc3x3_pad_asym", (8, 8, 16), 2, 20, 40, 3, 20, 22, pad=(1, 0), pad_bottom=(2, 3)),
    _row("pc3x3_sub_tile", (8, 8, 16), 2, 20, 40, 3, 6, 7),
    _row("pc3x3_tile_plus1", (8, 8, 16), 2, 20, 40, 3, 19, 35),       # 17 x 33 outputs: one past 2 x 2 tiles of 8 x 16
    _row("pc2x2_pad1_tile_plus1", (8, 8, 16), 2, 20, 40, 2, 8, 16, pad=(1, 1)),  # 9 x 17 outputs
    _row("pc1x1_pad1", (8, 8, 16), 2, 20, 75, 1, 13, 11, pad=(1, 1)),
    _row("pc1x1_circ1_tile_plus1", (8, 8, 16), 2, 36, 40, 1, 7, 15, circ=1),     # 9 x 17 outputs
    _row("gen5x5_circ2", (4, 16, 16), 2, 12, 16, 5, 19, 21, circ=2),
    _row("gen5x5_tile_plus1", (4, 16, 16), 2, 8, 12, 5, 21, 37, pad=(0, 0)),
    # ---- concatenated / cropped sources read by the kernel itself
    _row("pc3x3_src_16_16", (8, 8, 16), 2, ((16, 20, 20, 0, 0), (16, 20, 20, 0, 0)), 40, 3, 20, 20, circ=1),
    _row("pc3x3_src_20_12", (8, 8, 16), 2, ((20, 20, 20, 0, 0), (12, 20, 20, 0, 0)), 40, 3, 20, 20),
    _row("pc3x3_src_8_6_4", (8, 8, 16), 2, ((8, 20, 20, 0, 0), (6, 20, 20, 0, 0), (4, 20, 20, 0, 0)), 40, 3, 20, 20,
         pad=(1, 1)),
    _row("pc3x3_src_crop", (8, 8, 16), 2, _CROP, 40, 3, 20, 20, circ=1),
    _row("pc1x1_src_16_16", (8, 8, 16), 2, ((16, 20, 20, 0, 0), (16, 20, 20, 0, 0)), 75, 1, 20, 20),
    _row("pc1x1_src_20_12", (8, 8, 16), 2, ((20, 20, 20, 0, 0), (12, 20, 20, 0, 0)), 75, 1, 20, 20),
    _row("pc1x1_src_8_6_4", (8, 8, 16), 2, ((8, 20, 20, 0, 0), (6, 20, 20, 0, 0), (4, 20, 20, 0, 0)), 75, 1, 20, 20),
    _row("pc1x1_src_crop", (8, 8, 16), 2, _CROP, 200, 1, 20, 20),
    # ---- generic kernel only: fused prologue (padding stays 0, not act(GN(0))), dilation past the lattice, stride 2
    _row("gen5x5_gn1_gelu_pad2", (4, 16, 16), 2, 12, 16, 5, 19, 21, pad=(2, 2), gn=1, pre_act=1),
    _row("gen5x5_gn3_gelu_pad2", (4, 16, 16), 2, 12, 16, 5, 19, 21, pad=(2, 2), gn=3, pre_act=1),
    _row("gen5x5_gn1_gelu_crop", (4, 16, 16), 2, _CROP, 16, 5, 20, 20, pad=(2, 2), gn=1, pre_act=1),
    _row("gen5x5_gelu_only", (4, 16, 16), 2, 12, 16, 5, 19, 21, circ=2, pre_act=1),
    _row("gen5x5_dil8_circ", (4, 16, 16), 2, 8, 8, 5, 20, 20, dil=8, circ=16),
    _row("gen3x3_s2_c7_pad1", (2, 8, 16), 2, 7, 5, 3, 21, 22, stride=2, pad=(1, 1)),
]
FORWARD_CASES += _epilogues("pc3x3_epi", (8, 8, 16), 20, 40, 3, 20, 22, pad=(1, 1))
FORWARD_CASES += _epilogues("pc1x1_epi", (8, 8, 16), 36, 200, 1, 13, 11)
FORWARD_CASES += [
    _row("gen5x5_epi_nchw_os2", (4, 16, 16), 2, 12, 10, 5, 19, 21, pad=(2, 2), out_nchw=True, out_os=2, out_off=(1, 0),
         addends=1, act=1),
]
FORWARD_BY_NAME = {c.name: c for c in FORWARD_CASES}
assert len(FORWARD_BY_NAME) == len(FORWARD_CASES)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


class Inputs(NamedTuple):
    xs: tuple                   # sources, (B, C, H, W) fp32
    w: torch.Tensor             # (Cout, Cin, k, k)
    bias: Optional[torch.Tensor]
    gamma: Optional[torch.Tensor]
    beta: Optional[torch.Tensor]
    addends: tuple              # logical (B, out_C, out_H, out_W)
    prefill: torch.Tensor       # `out` before the launch, logical (B, out_C, out_H, out_W)


@functools.lru_cache(maxsize=None)
def forward_inputs(name) -> Inputs:
    c = FORWARD_BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(name))
    xs = tuple(torch.randn(c.B, s[0], s[1], s[2], generator=g) for s in c.srcs)
    w = torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g) / (c.Cin * c.k * c.k) ** 0.5
    bias = torch.randn(c.Cout, generator=g) if c.bias else None
    gamma = torch.rand(c.Cin, generator=g) + 0.5 if c.gn else None
    beta = torch.rand(c.Cin, generator=g) * 0.6 - 0.3 if c.gn else None
    addends = tuple(torch.randn(c.out_shape, generator=g) for _ in range(c.addends))
    return Inputs(xs, w, bias, gamma, beta, addends, torch.randn(c.out_shape, generator=g))


def _dest(c: Case):
    """(conv rows, dest rows, conv cols, dest cols) of the output pixels that land inside `out`."""
    Ho, Wo = c.conv_hw
    _, _, oh, ow = c.out_shape
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    dy, dx = oy * c.out_os + c.out_off[0], ox * c.out_os + c.out_off[1]
    my, mx = (dy >= 0) & (dy < oh), (dx >= 0) & (dx < ow)
    return oy[my], dy[my], ox[mx], dx[mx]


def touched_mask(c: Case) -> torch.Tensor:
    """bool (B, out_C, out_H, out_W): the elements of `out` the launch writes; all others must keep their bits"""
    m = torch.zeros(c.out_shape, dtype=torch.bool)
    _, dy, _, dx = _dest(c)
    m[:, :c.Cout, dy[:, None], dx[None, :]] = True
    return m


def forward_reference(c: Case, inp: Inputs, dtype) -> torch.Tensor:
    """`out` after the launch, logical (B, out_C, out_H, out_W), computed with torch on the CPU in `dtype`: the frame
    written out (crop / zero fill / concat), GroupNorm + GELU over it, circular wrap, zero padding, F.conv2d, and
    the epilogue act(acc + bias [+ addends]) [+ addends] [+ out] in plain torch."""
    H, W = c.frame
    parts = []
    for (C, h, w_, oy, ox), x in zip(c.srcs, inp.xs):
        f = torch.zeros(c.B, C, H, W, dtype=dtype)
        y0, y1, x0, x1 = max(0, oy), min(H, oy + h), max(0, ox), min(W, ox + w_)
        f[:, :, y0:y1, x0:x1] = x[:, :, y0 - oy:y1 - oy, x0 - ox:x1 - ox].to(dtype)
        parts.append(f)
    fr = torch.cat(parts, dim=1)
    if c.gn:
        fr = F.group_norm(fr, c.gn, inp.gamma.to(dtype), inp.beta.to(dtype), GN_EPS)
    if c.pre_act:
        fr = F.gelu(fr)
    if c.circ:
        fr = F.pad(fr, (c.circ,) * 4, mode="circular")
    pb = c.pad if c.pad_bottom is None else c.pad_bottom
    fr = F.pad(fr, (c.pad[1], pb[1], c.pad[0], pb[0]))
    r = F.conv2d(fr, inp.w.to(dtype), None, stride=c.stride, dilation=c.dil)
    assert tuple(r.shape[2:]) == c.conv_hw, (r.shape, c.conv_hw)
    out = inp.prefill.to(dtype).clone()
    oy, dy, ox, dx = _dest(c)
    iy, ix = dy[:, None], dx[None, :]
    v = r[:, :, oy[:, None], ox[None, :]]
    if inp.bias is not None:
        v = v + inp.bias.to(dtype).view(1, -1, 1, 1)
    ads = [a.to(dtype)[:, :c.Cout, iy, ix] for a in inp.addends]
    if not c.add_after_act:
        for a in ads:
            v = v + a
    if c.act:
        v = F.gelu(v)
    if c.add_after_act:
        for a in ads:
            v = v + a
    if c.accumulate:
        v = v + out[:, :c.Cout, iy, ix]
    out[:, :c.Cout, iy, ix] = v
    return out


@functools.lru_cache(maxsize=None)
def forward_refs(name):
    """(ref64, cpu32) of a row, computed once and shared (read-only)"""
    c, inp = FORWARD_BY_NAME[name], forward_inputs(name)
    return forward_reference(c, inp, torch.float64), forward_reference(c, inp, torch.float32)


def _layout(t, nchw):
    """logical (B, C, H, W) -> the device tensor in the launch's layout"""
    return (t if nchw else t.permute(0, 2, 3, 1)).contiguous().to(DEV)


def run_forward(c: Case):
    """The row on the GPU under the current precision.  Planned rows go through ops.pack_conv_weight / ops.conv2d with
    ops.conv_probe recording the launch; forced rows through a hand-filled nps_conv2d_t.  Returns (out as logical
    (B, out_C, out_H, out_W) on the CPU, [(arithmetic, taps, waves), ...] of the launches)."""
    import nps_hip
    from nps_hip import ops
    inp = forward_inputs(c.name)
    srcs = [ops.Src(_layout(x, False), s[3], s[4]) for s, x in zip(c.srcs, inp.xs)]
    wd = inp.w.to(DEV)
    bias = inp.bias.to(DEV) if inp.bias is not None else None
    out = _layout(inp.prefill, c.out_nchw)
    ads = [_layout(a, c.out_nchw) for a in inp.addends]
    gn = None
    if c.gn:
        gn = ops.GN(ops.group_norm_stats(srcs, c.frame, c.gn), inp.gamma.to(DEV), inp.beta.to(DEV), c.gn, GN_EPS)
    wp = ops.pack_conv_weight(wd, c.stride, c.dil)
    pb = c.pad if c.pad_bottom is None else c.pad_bottom
    if not c.forced:
        ops.conv_probe = []
        try:
            ops.conv2d(srcs, c.frame, wp, bias, c.Cout, c.k, c.k, stride=c.stride, dil=c.dil, pad=c.pad, circ=c.circ,
                       gn=gn, pre_act=c.pre_act, out=out, out_nchw=c.out_nchw, out_os=c.out_os, out_off=c.out_off,
                       accumulate=c.accumulate, addends=ads, act=c.act, add_after_act=c.add_after_act, pad_bottom=pb,
                       out_hw=c.conv_hw)
            launches = [p[3] for p in ops.conv_probe]
        finally:
            ops.conv_probe = None
    else:
        assert wp.nps_precision == ops.PREC_F32
        a = nps_hip.Conv2dArgs()
        a.nsrc = len(srcs)
        for i, s in enumerate(srcs):
            a.src[i].ptr, a.src[i].H, a.src[i].W, a.src[i].C = s.t.data_ptr(), s.t.shape[1], s.t.shape[2], s.t.shape[3]
            a.src[i].off_y, a.src[i].off_x = s.off_y, s.off_x
        a.B, a.Hin, a.Win, a.Cin = c.B, c.frame[0], c.frame[1], c.Cin
        if gn is not None:
            a.gn_stats, a.gn_gamma, a.gn_beta = gn.stats.data_ptr(), gn.gamma.data_ptr(), gn.beta.data_ptr()
            a.gn_groups, a.gn_eps = gn.groups, gn.eps
        a.pre_act = c.pre_act
        a.KH = a.KW = c.k
        a.stride, a.dil, a.pad_y, a.pad_x, a.circ = c.stride, c.dil, c.pad[0], c.pad[1], c.circ
        a.Hout, a.Wout = c.conv_hw
        a.wpack, a.bias, a.Cout = wp.data_ptr(), nps_hip.ptr(bias), c.Cout
        _, oC, oH, oW = c.out_shape
        a.out, a.out_C, a.out_H, a.out_W = out.data_ptr(), oC, oH, oW
        a.out_os, a.out_off_y, a.out_off_x = c.out_os, c.out_off[0], c.out_off[1]
        a.out_nchw, a.accumulate = int(c.out_nchw), int(c.accumulate)
        a.addend0 = ads[0].data_ptr() if len(ads) > 0 else None
        a.addend1 = ads[1].data_ptr() if len(ads) > 1 else None
        a.act, a.add_after_act = c.act, int(c.add_after_act)
        a.precision = ops.PREC_F32
        a.waves, a.TH, a.TW = c.plan
        a.lattice = 1 if (c.dil > 1 and c.stride == 1) else 0   # as nps_conv2d_plan sets it
        nps_hip.check(nps_hip.lib.nps_conv2d_fwd(ctypes.byref(a), nps_hip.stream_ptr()), "conv2d_fwd (caller's tile)")
        launches = [("f32", c.k * c.k, a.waves)]
    torch.cuda.synchronize()
    got = out.cpu()
    return (got if c.out_nchw else got.permute(0, 3, 1, 2)), launches


# --------------------------------------------------------------------------------------- weight gradient
class WCase(NamedTuple):
    name: str
    B: int
    M: int
    N: int
    k: int
    dil: int
    pad: int
    circ: int
    Ha: int
    Wa: int
    seeded: bool = False        # g given and nonzero: the kernel adds to it

    @property
    def x_hw(self):
        e = self.dil * (self.k - 1) - 2 * self.pad - 2 * self.circ
        return self.Ha + e, self.Wa + e


WGRAD_CASES = [
    # k = 1, 2, 3 with pad 0 / 1 and circ 0 / 1; M, N in {20, 64, 68, 132}: tails of both 64-tiles, n_mt, n_nt > 1
    WCase("k1", 2, 20, 64, 1, 1, 0, 0, 20, 24),
    WCase("k1_pad1", 2, 68, 132, 1, 1, 1, 0, 20, 24),
    WCase("k2_pad1", 2, 64, 68, 2, 1, 1, 0, 21, 19),
    WCase("k2_circ1", 2, 68, 20, 2, 1, 0, 1, 21, 19),
    WCase("k3", 2, 20, 20, 3, 1, 0, 0, 18, 22),
    WCase("k3_pad1", 2, 132, 64, 3, 1, 1, 0, 18, 22),
    WCase("k3_circ1", 2, 64, 132, 3, 1, 0, 1, 18, 22),
    # 5x5: 25 taps = tap groups of 9, 9 and 7; dilation 1, 2, 4 (A pixels on the dilation lattice)
    WCase("k5_pad2", 2, 20, 68, 5, 1, 2, 0, 19, 21),
    WCase("k5_dil2_circ4", 2, 68, 20, 5, 2, 0, 4, 24, 22),
    WCase("k5_dil4_pad8", 2, 64, 64, 5, 4, 8, 0, 20, 23),
    # channel counts off the 4-channel quads: the scalar ld4 branch
    WCase("k3_m30_n22", 2, 30, 22, 3, 1, 1, 0, 18, 22),
    WCase("k5_dil2_m30_n22", 2, 30, 22, 5, 2, 4, 0, 18, 22),
    # both ends of the split-K arithmetic: one pixel tile in total, many
    WCase("k3_one_tile", 1, 64, 64, 3, 1, 1, 0, 4, 16),
    WCase("k3_many_tiles", 3, 20, 132, 3, 1, 1, 0, 40, 36),
    WCase("k1_many_tiles", 3, 132, 68, 1, 1, 0, 0, 40, 36),
    # g given and nonzero
    WCase("k3_seeded", 2, 20, 64, 3, 1, 1, 0, 18, 22, True),
    WCase("k5_dil2_seeded", 2, 68, 20, 5, 2, 0, 4, 24, 22, True),
]
WGRAD_BY_NAME = {c.name: c for c in WGRAD_CASES}
assert len(WGRAD_BY_NAME) == len(WGRAD_CASES)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    """(a (B, M, Ha, Wa), x (B, N, Hx, Wx), g0 (M, N, k, k) or None), fp32"""
    c = WGRAD_BY_NAME[name]
    g = torch.Generator().manual_seed(_seed("wgrad_" + name))
    Hx, Wx = c.x_hw
    a = torch.randn(c.B, c.M, c.Ha, c.Wa, generator=g)
    x = torch.randn(c.B, c.N, Hx, Wx, generator=g)
    g0 = torch.randn(c.M, c.N, c.k, c.k, generator=g) * (c.B * c.Ha * c.Wa) ** 0.5 if c.seeded else None
    return a, x, g0


def wgrad_reference(c: WCase, dtype):
    a, x, g0 = wgrad_inputs(c.name)
    xe = x.to(dtype)
    if c.circ:
        xe = F.pad(xe, (c.circ,) * 4, mode="circular")
    xe = F.pad(xe, (c.pad,) * 4)
    r = torch.nn.grad.conv2d_weight(xe, (c.M, c.N, c.k, c.k), a.to(dtype), dilation=c.dil)
    return r + g0.to(dtype) if g0 is not None else r


@functools.lru_cache(maxsize=None)
def wgrad_refs(name):
    c = WGRAD_BY_NAME[name]
    return wgrad_reference(c, torch.float64), wgrad_reference(c, torch.float32)


def run_wgrad(c: WCase):
    """ad.wgrad on the GPU under the current precision: (g on the CPU, recorded launches)"""
    from nps_hip import autograd as ad
    from nps_hip import ops
    a, x, g0 = wgrad_inputs(c.name)
    ops.conv_probe = []
    try:
        g = ad.wgrad(_layout(a, False), _layout(x, False), c.k, c.k, dil=c.dil, pad=(c.pad, c.pad), circ=c.circ,
                     g=g0.to(DEV) if g0 is not None else None)
        launches = [p[3] for p in ops.conv_probe]
    finally:
        ops.conv_probe = None
    torch.cuda.synchronize()
    return g.cpu(), launches


def rel_l2_on(a, b, mask=None):
    """rel-L2 of a against b in fp64, over `mask` only when given"""
    a, b = a.to(torch.float64), b.to(torch.float64)
    if mask is not None:
        a, b = a[mask], b[mask]
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()
