"""The 3-D conv forward (csrc/conv3d.hip, nps_conv3d_fwd / nps_frame_pack3d / nps_gn_stats3d / nps_conv3d_pack_weights)
restated in fp64 torch on the CPU, the case tables with the kernel instantiation each row is meant to reach, and the
elementwise error bound.  No tests here: tests/test_conv3d_ref_host.py (no GPU) and tests/test_gpu_conv3d_fwd.py use it.

nps_conv3d_fwd launches (names as nps_conv3d_route gives them)
  conv3d_kernel<T,K,S,TH,SIMPLE|GENERAL,FORM>   T in {f32, bf16}, (K,S,TH) in {(3,1,8), (3,2,4), (2,1,8), (1,1,8)};
      SIMPLE: one 16-channel-aligned source covering the frame, no prologue; GENERAL: load_piece over up to three
      sources + the fused GroupNorm / GELU prologue.  FORM: REG everywhere in fp32; in bf16 DMA (K = 3) / DMA_O4 (K = 2)
      on SIMPLE frames, REG_O4 for the GENERAL 1x1x1, REG otherwise
  conv3d_1x1_kernel<NCB,NCH,PRO|PLAIN>          bf16 1x1x1 over <= 2 sources, Cout <= 128 (NCB 2 / 4), Cin <= 256
      (NCH 5 / 9 / 16 K-step register sets)

The reference of a row: frame() (crop_Nd / torch.cat) -> prologue() on core-frame values, uncovered zeros included ->
extend() circular then zeros (so the wrapped halo holds normalised values and the zero padding stays zero) -> F.conv3d
(F.conv_transpose3d(k = 4, s = 2) when transposed) -> bias + addend -> act -> + old where it accumulates, placed at
m * out_os + out_off inside the (out_D, out_H, out_W, out_C) destination.  bf16 rows round every operand the kernel
reads from memory to bf16 first (_rt); the only difference left is the rounding of the stored value.

Elementwise bound (rows without activation and prologue), derived, not measured:
    |y - ref| <= u |ref| + (1 + u) (n + 3) 2^-24 A,   n = Cin K^3,   A = abs_sum() = the same conv over |x|, |w|,
    |bias|, |addend|;   u = 0 (fp32), 2^-8 (bf16: the one round-to-nearest of the stored value)
(n products summed in fp32 in any order, bias, addend and the old value added in fp32: n + 2 roundings of partial sums
each <= 2^-24 of a value bounded by A, to first order; + 1 covers the second-order terms at these n.)"""
import ctypes
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

GN_EPS = 1e-5
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}     # the project's bars (tests/test_gpu_conv3d.py)
UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
GEO = {(3, 1): 8, (3, 2): 4, (2, 1): 8, (1, 1): 8}    # (K, stride) -> TH


# ------------------------------------------------------------------------------------------- the fp64 restatement
def _rt(x, dt):
    """the operand as the kernel sees it (bf16-rounded for bf16 storage)."""
    return x.to(dt).double() if dt == torch.bfloat16 else x.double()


def frame(srcs, B, dhw):
    """torch.cat of crop_Nd-placed sources (NCDHW, the sources' dtype); srcs = [(tensor, (off_d, off_h, off_w)), ...]"""
    C = sum(s.shape[1] for s, _ in srcs)
    fr = torch.zeros(B, C, *dhw, dtype=srcs[0][0].dtype)
    c = 0
    for s, off in srcs:
        D, H, W = s.shape[2:]
        lo = [max(0, o) for o in off]
        hi = [min(n, o + m) for n, o, m in zip(dhw, off, (D, H, W))]
        if all(h > l for l, h in zip(lo, hi)):
            fr[:, c:c + s.shape[1], lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = \
                s[:, :, lo[0] - off[0]:hi[0] - off[0], lo[1] - off[1]:hi[1] - off[1], lo[2] - off[2]:hi[2] - off[2]]
        c += s.shape[1]
    return fr


def extend(fr, circ, zpad):
    """circular first, then zeros, per side of every spatial axis"""
    if circ:
        fr = F.pad(fr, (circ,) * 6, mode="circular")
    if zpad:
        fr = F.pad(fr, (zpad,) * 6)
    return fr


def prologue(fr, gn, pre_act):
    """act(GN(core frame)); gn = (groups, gamma, beta) or None"""
    if gn is not None:
        fr = F.group_norm(fr, gn[0], gn[1].to(fr.dtype), gn[2].to(fr.dtype), eps=GN_EPS)
    if pre_act:
        fr = F.gelu(fr)
    return fr


def conv(fr_ext, w, bias, K, stride=1, transposed=False):
    """fr_ext: the extended frame (without the last zero voxel per side when transposed: ConvTranspose3d's full output
    is the valid 2^3-phase conv over one more zero voxel).  (B, Cout, Dout, Hout, Wout), phases interleaved."""
    if transposed:
        return F.conv_transpose3d(fr_ext, w, bias, stride=2)
    return F.conv3d(fr_ext, w, bias, stride=stride)


class Case(NamedTuple):
    name: str
    routes: tuple                    # ((dtype name, route), ...): the instantiation the row is meant to reach
    B: int
    srcs: tuple                      # ((C, D, H, W, off_d, off_h, off_w), ...)
    dhw: Tuple[int, int, int]        # core frame
    Cout: int
    K: int
    stride: int = 1
    transposed: bool = False
    circ: int = 0
    zpad: int = 0
    gn: int = 0                      # GroupNorm groups of the prologue (0: none)
    pre_act: int = 0
    bias: bool = True
    act: int = 0
    addend: bool = False
    accumulate: bool = False
    out_C: Optional[int] = None
    out_os: int = 1                  # (ignored when transposed: 2)
    out_off: Tuple[int, int, int] = (0, 0, 0)
    out_dhw: Optional[Tuple[int, int, int]] = None
    pack: bool = True                # ops.CONV3D_PACK during the launch
    grid: int = 0                    # nps_conv3d_1x1_set_grid during the launch
    stats: bool = False              # pass out_stats

    @property
    def Cin(self):
        return sum(s[0] for s in self.srcs)

    @property
    def ext_dhw(self):
        return tuple(n + 2 * (self.circ + self.zpad) for n in self.dhw)

    @property
    def conv_dhw(self):
        """conv output positions per phase (nps_conv3d_t.Dout, Hout, Wout)"""
        return tuple((n - self.K) // self.stride + 1 for n in self.ext_dhw)

    @property
    def space(self):
        """the conv's output space: phases interleaved when transposed"""
        return tuple((2 if self.transposed else 1) * n for n in self.conv_dhw)

    @property
    def os(self):
        """destination stride per index of `space`"""
        return 1 if self.transposed else self.out_os

    @property
    def out_shape(self):
        """logical (B, out_C, out_D, out_H, out_W)"""
        d = self.out_dhw if self.out_dhw is not None else tuple(self.os * n for n in self.space)
        return (self.B, self.out_C or self.Cout) + tuple(d)

    @property
    def partial(self):
        """the launch leaves part of `out` alone (or reads it): `out` is pre-filled with a pattern, not NaN"""
        return self.accumulate or not bool(touched_mask(self).all())

    @property
    def plain(self):
        """no activation and no prologue: judged by the elementwise bound too"""
        return not (self.act or self.gn or self.pre_act)

    def route(self, dt):
        return dict(self.routes).get(dt)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


class Inputs(NamedTuple):
    xs: tuple                    # sources, (B, C, D, H, W) fp32
    w: torch.Tensor              # (Cout, Cin, K, K, K), or (Cin, Cout, 4, 4, 4) transposed
    bias: Optional[torch.Tensor]
    gamma: Optional[torch.Tensor]
    beta: Optional[torch.Tensor]
    addend: Optional[torch.Tensor]   # logical out_shape
    prefill: torch.Tensor            # `out` before the launch where the row is `partial`, logical out_shape


@functools.lru_cache(maxsize=None)
def inputs(name) -> Inputs:
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(name))
    # (a mean per source, so the GroupNorm has something to remove and an uncovered voxel normalises to a value that
    # is visibly not zero)
    xs = tuple(torch.randn(c.B, s[0], *s[1:4], generator=g) * (1 + 0.5 * k) + 0.4 * (k + 1) for k, s in enumerate(c.srcs))
    n = c.Cin * c.K ** 3
    wshape = (c.Cin, c.Cout, 4, 4, 4) if c.transposed else (c.Cout, c.Cin, c.K, c.K, c.K)
    w = torch.randn(wshape, generator=g) / n ** 0.5
    bias = torch.randn(c.Cout, generator=g) * 0.5 if c.bias else None
    gamma = torch.rand(c.Cin, generator=g) + 0.5 if c.gn else None
    beta = (torch.rand(c.Cin, generator=g) * 0.6 + 0.2) * (1 - 2 * (torch.arange(c.Cin) % 2)) if c.gn else None
    addend = torch.randn(c.out_shape, generator=g) if c.addend else None
    return Inputs(xs, w, bias, gamma, beta, addend, torch.randn(c.out_shape, generator=g))


def _dest(c: Case):
    """per axis: (indices of the conv's output space, their destination indices) that land inside `out`"""
    res = []
    for n, off, lim in zip(c.space, c.out_off, c.out_shape[2:]):
        j = torch.arange(n)
        d = j * c.os + off
        m = (d >= 0) & (d < lim)
        res.append((j[m], d[m]))
    return res


def touched_mask(c: Case) -> torch.Tensor:
    """bool out_shape: the elements of `out` the launch writes; every other one must keep its bits"""
    m = torch.zeros(c.out_shape, dtype=torch.bool)
    (_, dd), (_, dh), (_, dw) = _dest(c)
    m[:, :c.Cout, dd[:, None, None], dh[None, :, None], dw[None, None, :]] = True
    return m


def window(c: Case, out):
    """the written window of a logical out_shape tensor, (B, Cout, nd, nh, nw)"""
    (_, dd), (_, dh), (_, dw) = _dest(c)
    return out[:, :c.Cout, dd[:, None, None], dh[None, :, None], dw[None, None, :]]


def _operands(c: Case, inp: Inputs, dt, absolute, compute=torch.float64):
    f = (lambda t: _rt(t, dt).abs().to(compute)) if absolute else (lambda t: _rt(t, dt).to(compute))
    fr = frame([(f(x), s[4:7]) for x, s in zip(inp.xs, c.srcs)], c.B, c.dhw)
    if not absolute:
        gn = (c.gn, inp.gamma, inp.beta) if c.gn else None
        fr = prologue(fr, gn, c.pre_act)
        if c.gn or c.pre_act:
            fr = _rt(fr, dt).to(compute)     # bf16: the kernel rounds the normalised frame to bf16 once more (the LDS image)
    else:
        assert c.plain
    fr = extend(fr, c.circ, c.zpad - 1 if c.transposed else c.zpad)
    bias = None if inp.bias is None else (inp.bias.abs() if absolute else inp.bias).to(compute)
    r = conv(fr, f(inp.w), bias, c.K, c.stride, c.transposed)
    assert tuple(r.shape[2:]) == c.space, (r.shape, c.space)
    (jd, _), (jh, _), (jw, _) = _dest(c)
    v = r[:, :, jd[:, None, None], jh[None, :, None], jw[None, None, :]]
    if inp.addend is not None:
        v = v + window(c, f(inp.addend))
    return v


def reference(c: Case, dt, compute=torch.float64) -> torch.Tensor:
    """`out` after the launch, logical out_shape, computed in `compute` (fp64: the reference) from the operands as
    the kernel reads them.  Elements the launch does not write hold the pre-fill (as stored: rounded to dt)."""
    inp = inputs(c.name)
    v = _operands(c, inp, dt, False, compute)
    if c.act:
        v = F.gelu(v)
    out = _rt(inp.prefill, dt).to(compute)
    if c.accumulate:
        v = v + window(c, out)
    (_, dd), (_, dh), (_, dw) = _dest(c)
    out[:, :c.Cout, dd[:, None, None], dh[None, :, None], dw[None, None, :]] = v
    return out


def abs_sum(c: Case, dt) -> torch.Tensor:
    """A of the bound on the written window, (B, Cout, nd, nh, nw): the row's conv over |x|, |w|, |bias|, |addend|"""
    return _operands(c, inputs(c.name), dt, True)


def bound(c: Case, dt) -> torch.Tensor:
    """the elementwise bound on the written window (module docstring)"""
    u = UNIT[dt]
    n = c.Cin * c.K ** 3
    return u * window(c, refs(c.name, dt)).abs() + (1 + u) * (n + 3) * 2.0 ** -24 * abs_sum(c, dt)


@functools.lru_cache(maxsize=None)
def refs(name, dt):
    """a row's reference, computed once and shared (read-only)"""
    return reference(BY_NAME[name], dt)


# ------------------------------------------------------------------------------------------- routes
def R(T, K, S, simple, form="REG"):
    return f"conv3d_kernel<{T},{K},{S},{GEO[(K, S)]},{'SIMPLE' if simple else 'GENERAL'},{form}>"


def R1(ncb, nch, pro):
    return f"conv3d_1x1_kernel<{ncb},{nch},{'PRO' if pro else 'PLAIN'}>"


# Every instantiation nps_conv3d_fwd can launch in the default build with no environment knob set, and (the GENERAL
# K > 1 ones) with ops.CONV3D_PACK off.  Left to test_gpu_conv3d.py's child-process bit-equality test, because an
# environment knob read once per process selects them and they are pinned bit for bit against the routes below:
#   NPS_C3D_GLDS=0: conv3d_kernel<bf16,3,1,8,SIMPLE,REG>, <bf16,3,2,4,SIMPLE,REG>, <bf16,2,1,8,SIMPLE,REG>
#   NPS_C3D_K1O4=0: conv3d_kernel<bf16,1,1,8,GENERAL,REG>
ALL_ROUTES = frozenset(
    [R("f32", K, S, sim) for (K, S) in GEO for sim in (True, False)] +
    [R("bf16", 3, 1, True, "DMA"), R("bf16", 3, 2, True, "DMA"), R("bf16", 2, 1, True, "DMA_O4"), R("bf16", 1, 1, True),
     R("bf16", 3, 1, False), R("bf16", 3, 2, False), R("bf16", 2, 1, False), R("bf16", 1, 1, False, "REG_O4")] +
    [R1(ncb, nch, pro) for ncb in (2, 4) for nch in (5, 9, 16) for pro in (False, True)])


def _both(K, S, simple, bf16_form="REG"):
    return (("f32", R("f32", K, S, simple)), ("bf16", R("bf16", K, S, simple, bf16_form)))


def launch_args(c: Case, dt):
    """The nps_conv3d_t ops.conv3d fills for the row (dummy pointers: for nps_conv3d_route, host arithmetic only).
    With ops.CONV3D_PACK on, a K > 1 conv whose frame is not SIMPLE reads the frame_pack3d output instead."""
    import nps_hip
    srcs, gn, pre_act = c.srcs, c.gn, c.pre_act
    simple = (len(srcs) == 1 and not gn and not pre_act and tuple(srcs[0][1:4]) == tuple(c.dhw)
              and not any(srcs[0][4:7]) and srcs[0][0] % 16 == 0)
    if c.pack and c.K > 1 and not simple:
        srcs, gn, pre_act = (((c.Cin + 15) // 16 * 16,) + tuple(c.dhw) + (0, 0, 0),), 0, 0
    a = nps_hip.Conv3dArgs()
    a.nsrc = len(srcs)
    for i, s in enumerate(srcs):
        a.src[i].ptr = 0x10000 * (i + 1)
        a.src[i].C, a.src[i].D, a.src[i].H, a.src[i].W, a.src[i].off_d, a.src[i].off_h, a.src[i].off_w = s
    a.B, (a.Dc, a.Hc, a.Wc), a.Cin = c.B, c.dhw, sum(s[0] for s in srcs)
    a.bf16 = int(dt == torch.bfloat16)
    a.circ, a.zpad = c.circ, c.zpad
    if gn:
        a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_groups, a.gn_eps = 0x80000, 0x90000, 0xa0000, gn, GN_EPS
    a.pre_act = pre_act
    a.K, a.stride, a.transposed = c.K, c.stride, int(c.transposed)
    a.Dout, a.Hout, a.Wout = c.conv_dhw
    a.wpack, a.bias, a.Cout = 0xb0000, (0xc0000 if c.bias else None), c.Cout
    _, a.out_C, a.out_D, a.out_H, a.out_W = c.out_shape
    a.out, a.out_os = 0xd0000, (2 if c.transposed else c.out_os)
    a.out_off_d, a.out_off_h, a.out_off_w = c.out_off
    a.accumulate, a.addend, a.act = int(c.accumulate), (0xe0000 if c.addend else None), c.act
    a.out_stats = 0xf0000 if c.stats else None
    return a


def route_of(a) -> str:
    """nps_conv3d_route of a filled nps_conv3d_t"""
    import nps_hip
    buf = ctypes.create_string_buffer(96)
    if nps_hip.lib.nps_conv3d_route(ctypes.byref(a), buf, len(buf)) < 0:
        raise RuntimeError("conv3d_route: " + nps_hip.lib.nps_last_error().decode())
    return buf.value.decode()


# ------------------------------------------------------------------------------------------- the rows
def _one(C, dhw):
    return ((C,) + tuple(dhw) + (0, 0, 0),)


def _row(name, routes, srcs, dhw, Cout, K, **kw):
    return Case(name, tuple(routes), 2, tuple(srcs), tuple(dhw), Cout, K, **kw)


# Geometry of every conv row: B = 2, Dout >= 2, Hout = TH + 1 (a second row tile of one row), Wout in [33, 40] (a second
# 32-column tile with a tail), Cout 68 / 70 (4 / 6 channels in a second 64-channel tile).  That makes B Dout 2 2 tiles,
# always a multiple of 8, so the "_rem" row of each kernel family has Dout = 3 and Hout = 2 TH + 1 instead: 36 work-
# groups, of which the last 4 are the remainder the XCD remap leaves where they are.
SIMPLE_ROWS = [
    _row("s_k3s1_valid_rem", _both(3, 1, True, "DMA"), _one(32, (5, 19, 37)), (5, 19, 37), 68, 3),
    _row("s_k3s1_zpad1", _both(3, 1, True, "DMA"), _one(32, (2, 9, 35)), (2, 9, 35), 70, 3, zpad=1),
    _row("s_k3s1_circ1", _both(3, 1, True, "DMA"), _one(32, (2, 9, 35)), (2, 9, 35), 68, 3, circ=1),
    _row("s_k3s1_circ1_zpad1", _both(3, 1, True, "DMA"), _one(32, (2, 7, 33)), (2, 7, 33), 70, 3, circ=1, zpad=1),
    _row("s_k3s2_valid_rem", _both(3, 2, True, "DMA"), _one(32, (7, 19, 69)), (7, 19, 69), 68, 3, stride=2),
    _row("s_k3s2_zpad1", _both(3, 2, True, "DMA"), _one(32, (3, 9, 67)), (3, 9, 67), 70, 3, stride=2, zpad=1),
    _row("s_k2s1_rem", _both(2, 1, True, "DMA_O4"), _one(32, (4, 18, 36)), (4, 18, 36), 68, 2),
    # the 3-D Upsample: circular pad 1, ConvTranspose3d(k 4, s 2) = 8 phase convs (K = 2) over one more zero voxel
    _row("s_k2_transposed", _both(2, 1, True, "DMA_O4"), _one(32, (2, 6, 32)), (2, 6, 32), 68, 2, transposed=True,
         circ=1, zpad=1),
    _row("s_k1_f32_rem", (("f32", R("f32", 1, 1, True)),), _one(32, (3, 17, 35)), (3, 17, 35), 68, 1),
    # Cout > 128: past the bf16 1x1x1 kernel
    _row("s_k1_bf16_cout132", (("bf16", R("bf16", 1, 1, True)),), _one(32, (3, 17, 35)), (3, 17, 35), 132, 1),
]

# (8, 5, 3) channels: a whole-piece source, an element-load source (C % 4 != 0), a half straddling a source boundary;
# (4, 8, 4): 4-channel halves (load_half).  Crop offsets of both signs on every axis, uncovered voxels.
def _frames(dhw, last=3):
    D, H, W = dhw
    crop = lambda C, o: (C,) + tuple(n - 2 * oo if n - 2 * oo > 0 else 1 for n, oo in zip(dhw, o)) + tuple(o)
    a = ((8, D, H, W, 0, 0, 0), crop(5, (-1, 1, -2)), crop(last, (1, -1, 2)))
    b = ((4, D, H, W, 0, 0, 0), crop(8, (1, -2, 1)), crop(4, (-1, 1, -1)))
    return a, b


_GEN1 = _both(1, 1, False, "REG_O4")
_FA, _FB = _frames((2, 9, 35))
_FA3, _FB3 = _frames((3, 17, 35))
GENERAL_K1_ROWS = [
    _row("g_k1_853_rem", _GEN1, _FA3, (3, 17, 35), 6, 1, out_C=10),
    _row("g_k1_853_gn2_gelu", _GEN1, _FA, (2, 9, 35), 6, 1, out_C=10, gn=2, pre_act=1),
    _row("g_k1_484", _GEN1, _FB, (2, 9, 35), 8, 1),
    _row("g_k1_484_gn2_gelu", _GEN1, _FB, (2, 9, 35), 8, 1, gn=2, pre_act=1),
    # (8, 5, 7) = 20 channels: the prologue on a partial last 16-channel chunk
    _row("g_k1_857_gn2_gelu", _GEN1, _frames((2, 9, 35), 7)[0], (2, 9, 35), 6, 1, out_C=10, gn=2, pre_act=1),
]

# the fused GENERAL kernels for K > 1: reached with ops.CONV3D_PACK off (include/nps.h documents nps_conv3d_fwd so)
_F31A, _F31B = _frames((2, 7, 33))
_F32A, _F32B = _frames((3, 9, 67))
_F21A, _F21B = _frames((2, 6, 32))
_F31R, _ = _frames((3, 15, 33))
GENERAL_KN_ROWS = [
    _row("g_k3s1_853_gn2_gelu", _both(3, 1, False), _F31A, (2, 7, 33), 70, 3, circ=1, zpad=1, gn=2, pre_act=1, pack=False),
    _row("g_k3s1_484_gn2_gelu", _both(3, 1, False), _F31B, (2, 7, 33), 8, 3, circ=1, zpad=1, gn=2, pre_act=1, pack=False),
    _row("g_k3s1_857_gn2_gelu", _both(3, 1, False), _frames((2, 7, 33), 7)[0], (2, 7, 33), 70, 3, circ=1, zpad=1, gn=2,
         pre_act=1, pack=False),
    _row("g_k3s1_853_plain_rem", _both(3, 1, False), _F31R, (3, 15, 33), 70, 3, circ=1, zpad=1, pack=False),
    _row("g_k3s2_853_gn2_gelu", _both(3, 2, False), _F32A, (3, 9, 67), 70, 3, stride=2, zpad=1, gn=2, pre_act=1, pack=False),
    _row("g_k3s2_484_gn2_gelu", _both(3, 2, False), _F32B, (3, 9, 67), 8, 3, stride=2, zpad=1, gn=2, pre_act=1, pack=False),
    _row("g_k2s1_853_gn2_gelu", _both(2, 1, False), _F21A, (2, 6, 32), 70, 2, circ=1, zpad=1, gn=2, pre_act=1, pack=False),
    _row("g_k2s1_484_gn2_gelu", _both(2, 1, False), _F21B, (2, 6, 32), 8, 2, circ=1, zpad=1, gn=2, pre_act=1, pack=False),
]

# conv3d_1x1_kernel: 945 voxels = 29 tiles of 32 and one of 17; the second source zero-padded on one axis and cropped on
# another.  Cin 204 = (192, 12): the last K-step's second half is past Cin, its first half an 8-B load at the source's end.
_V = (3, 9, 35)


def _two(c0, c1):
    return ((c0,) + _V + (0, 0, 0), (c1, 3, 7, 37, 0, 1, -1))


ONE_BY_ONE_ROWS = [
    _row(f"k1x1_{c0 + c1}_{cout}_{'pro' if pro else 'plain'}", (("bf16", R1(2 if cout <= 64 else 4, nch, pro)),),
         _two(c0, c1), _V, cout, 1, gn=2 * pro, pre_act=pro, stats=True)
    for (c0, c1, nch) in ((64, 4, 5), (128, 4, 9), (192, 12, 16)) for cout in (36, 100) for pro in (0, 1)]
# 2 work-groups per sample: 8 waves over 30 tiles, so six waves walk 4 tiles and two walk 3 (a ragged last round)
ONE_BY_ONE_ROWS += [
    _row(f"k1x1_68_36_{'pro' if pro else 'plain'}_grid2", (("bf16", R1(2, 5, pro)),), _two(64, 4), _V, 36, 1, gn=2 * pro,
         pre_act=pro, stats=True, grid=2) for pro in (0, 1)]


def _epilogues(tag, routes, srcs, dhw, Cout, K, **geo):
    """the epilogue matrix on one store path; every row passes out_stats"""
    base = Case(tag, tuple(routes), 2, tuple(srcs), tuple(dhw), Cout, K, stats=True, **geo)
    sp = base.space
    return [
        base._replace(name=f"{tag}_nobias", bias=False),
        base._replace(name=f"{tag}_bias"),
        base._replace(name=f"{tag}_addend", addend=True),
        base._replace(name=f"{tag}_addend_gelu", addend=True, act=1),
        base._replace(name=f"{tag}_accumulate", accumulate=True),
        base._replace(name=f"{tag}_accumulate_addend_gelu", accumulate=True, addend=True, act=1),
        # a negative offset into a smaller destination (crop) and a positive one into a larger (the rest keeps its bits)
        base._replace(name=f"{tag}_off_neg_crop", out_off=(-1, -2, -3), out_dhw=(sp[0] - 1, sp[1] - 3, sp[2] - 5), addend=True),
        base._replace(name=f"{tag}_off_pos_larger", out_off=(1, 2, 3), out_dhw=(sp[0] + 2, sp[1] + 3, sp[2] + 4), accumulate=True),
        base._replace(name=f"{tag}_os2", out_os=2, out_off=(1, 0, 1)),
    ]


EPILOGUE_ROWS = (
    _epilogues("e_f32_vec4", (("f32", R("f32", 3, 1, True)),), _one(16, (4, 11, 37)), (4, 11, 37), 8, 3) +
    _epilogues("e_bf16_vec4", (("bf16", R("bf16", 3, 1, True, "DMA")),), _one(16, (4, 11, 37)), (4, 11, 37), 8, 3) +
    _epilogues("e_elem", _GEN1, _FA, (2, 9, 35), 6, 1, out_C=10) +
    _epilogues("e_k1x1", (("bf16", R1(2, 5, False)),), ((16,) + _V + (0, 0, 0), (4, 3, 7, 37, 0, 1, -1)), _V, 8, 1))

CONV_ROWS = SIMPLE_ROWS + GENERAL_K1_ROWS + GENERAL_KN_ROWS + ONE_BY_ONE_ROWS + EPILOGUE_ROWS
BY_NAME = {c.name: c for c in CONV_ROWS}
assert len(BY_NAME) == len(CONV_ROWS)
CONV_PARAMS = [(c.name, dt) for c in CONV_ROWS for dt, _ in c.routes]


# ------------------------------------------------------------------------------------------- frames: moments and pack
class FrameCase(NamedTuple):
    name: str
    srcs: tuple
    dhw: Tuple[int, int, int]
    B: int = 2

    @property
    def Cin(self):
        return sum(s[0] for s in self.srcs)


_PA, _PB = _frames((4, 6, 11))
_INSIDE = lambda fr: tuple((s[0], 4, 6, 11, 0, 0, 0) for s in fr)
FRAME_CASES = [FrameCase("f853_inside", _INSIDE(_PA), (4, 6, 11)), FrameCase("f853_crop", _PA, (4, 6, 11)),
               FrameCase("f484_inside", _INSIDE(_PB), (4, 6, 11)), FrameCase("f484_crop", _PB, (4, 6, 11)),
               # C % 8 == 4 and C % 4 != 0 single sources
               FrameCase("f20_single", ((20, 4, 6, 11, 0, 0, 0),), (4, 6, 11)),
               FrameCase("f12_single_crop", ((12, 6, 4, 9, -1, 1, 2),), (4, 6, 11)),
               # 516 channels, packed to 528 > 512 (the up-block frame of a hidden-64 U-Net with ch_mults (2, 2) and
               # n_cond 4): past the one-thread-per-piece kernel's 64 pieces; whole sources, and skip / vb zero-padded in
               FrameCase("f516_inside", tuple((C, 3, 4, 5, 0, 0, 0) for C in (256, 256, 4)), (3, 4, 5)),
               FrameCase("f516_crop", ((256, 3, 4, 5, 0, 0, 0), (256, 2, 3, 4, 0, 1, 1), (4, 2, 3, 3, 1, 0, 2)),
                         (3, 4, 5))]
FRAME_BY_NAME = {c.name: c for c in FRAME_CASES}


@functools.lru_cache(maxsize=None)
def frame_inputs(name):
    """(sources (B, C, D, H, W) fp32, gamma, beta)"""
    c = FRAME_BY_NAME[name]
    g = torch.Generator().manual_seed(_seed("frame_" + name))
    xs = tuple(torch.randn(c.B, s[0], *s[1:4], generator=g) * (1 + 0.5 * k) + 0.4 * (k + 1) for k, s in enumerate(c.srcs))
    return xs, torch.rand(c.Cin, generator=g) + 0.5, torch.rand(c.Cin, generator=g) * 0.6 + 0.2


def frame_of(c: FrameCase, dt):
    xs, _, _ = frame_inputs(c.name)
    return frame([(_rt(x, dt), s[4:7]) for x, s in zip(xs, c.srcs)], c.B, c.dhw)


# ------------------------------------------------------------------------------------------- weight packing
# (Cout, Cin, K, transposed); the last: 2 211 840 packed elements, more than the 8192 x 256 threads of the pack grid
PACK_CASES = [(70, 20, 3, False), (6, 5, 1, False), (40, 48, 2, True), (512, 160, 3, False)]


def pack_weight_reference(w, K, transposed):
    """include/nps.h: [phase][64-channel Cout tile][kd][16-channel Cin chunk][kh][kw][64][16], zero padded; phase
    (pd, ph, pw) of a transposed conv takes kernel index p + 2 (1 - t) at tap t of an axis.  fp32, flat."""
    if transposed:
        Cin, Cout = w.shape[:2]
        t = torch.arange(2)
        phases = []
        for z in range(8):
            qd, qh, qw = ((z >> 2) & 1) + 2 * (1 - t), ((z >> 1) & 1) + 2 * (1 - t), (z & 1) + 2 * (1 - t)
            phases.append(w[:, :, qd[:, None, None], qh[None, :, None], qw[None, None, :]].transpose(0, 1))
        eff = torch.stack(phases)                                   # (8, Cout, Cin, 2, 2, 2)
    else:
        Cout, Cin = w.shape[:2]
        eff = w[None]
    ntile, nchunk = (Cout + 63) // 64, (Cin + 15) // 16
    full = torch.zeros(eff.shape[0], ntile * 64, nchunk * 16, K, K, K)
    full[:, :Cout, :Cin] = eff
    v = full.view(-1, ntile, 64, nchunk, 16, K, K, K)               # z tile col chunk k kd kh kw
    return v.permute(0, 1, 5, 3, 6, 7, 2, 4).contiguous().view(-1)  # z tile kd chunk kh kw col k
