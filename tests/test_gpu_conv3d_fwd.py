"""The 3-D conv forward kernels (csrc/conv3d.hip) pinned to the fp64 restatement of tests/conv3d_ref.py, one row per
dispatch route (conv3d_ref.ALL_ROUTES; tests/test_conv3d_ref_host.py proves the coverage without a GPU, and every row
here asserts the route its own launch took through nps_conv3d_route).

Every output lies between two guard rows of sentinel words.  A destination the launch writes in full is NaN-filled
first; one it writes in part (a crop window, out_os = 2, channels < out_C) or reads (accumulate) holds a random pattern,
and everything outside the written window must come back bit-unchanged.

Bars: the elementwise bound of conv3d_ref (rows with no activation and no prologue) and, for every row, rel-L2 < 1e-5
(fp32) / 1e-2 (bf16) on the whole written window and on each of its slices along the channel, d, h and w axes.  Rows
with a GELU or a prologue are judged by the slice bar alone: the accuracy of gelu_erf / gelu_fast is not measured, and
a bf16 re-rounding of the normalised operand can flip by one ulp.  Measured values: profiles/conv3d_fwd/README.md."""
import ctypes

import pytest
import torch

import conv3d_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                      # elements per guard row: keeps the body 128-B aligned
SENTINEL = {torch.float32: (torch.int32, 0x5A5A5A5A), torch.bfloat16: (torch.int16, 0x5A5A)}


class Guarded:
    """A device tensor of `shape` between two guard rows of sentinel words: NaN-filled, or holding `fill`."""

    def __init__(self, shape, dt, fill=None):
        n = 1
        for s in shape:
            n *= int(s)
        self.words, self.sentinel = SENTINEL[dt]
        self.buf = torch.empty(n + 2 * GUARD, dtype=dt, device=DEV)
        self.buf.view(self.words).fill_(self.sentinel)
        body = self.buf[GUARD:GUARD + n]
        if fill is None:
            body.fill_(float("nan"))
        else:
            body.copy_(fill.reshape(-1))
        self.t = body.view(*shape)

    def assert_guards(self):
        torch.cuda.synchronize()
        w = self.buf.view(self.words)
        assert bool((w[:GUARD] == self.sentinel).all()), "the guard row before the output was written"
        assert bool((w[-GUARD:] == self.sentinel).all()), "the guard row after the output was written"


def _ndhwc(x, dt):
    return x.permute(0, 2, 3, 4, 1).contiguous().to(dt)


def _logical(y):
    """device NDHWC -> CPU (B, C, D, H, W) in the storage dtype"""
    return y.cpu().permute(0, 4, 1, 2, 3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _slice_errors(got, ref):
    """(whole rel-L2, worst slice rel-L2, its (dim, index)) over the slices along dims 1..4"""
    whole = rel_l2(got, ref)
    worst, where = 0.0, None
    for dim in range(1, 5):
        num = (got - ref).square().sum([d for d in range(5) if d != dim]).sqrt()
        den = ref.square().sum([d for d in range(5) if d != dim]).sqrt()
        e = num / den
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        i = int(e.argmax())
        if e[i].item() >= worst:
            worst, where = e[i].item(), (dim, i)
    return whole, worst, where


def _run(c, dt, monkeypatch):
    """the row on the GPU: (Guarded out, out_stats buffer or None, [route of every nps_conv3d_fwd launch])"""
    import nps_hip
    from nps_hip import ops
    bf = dt == torch.bfloat16
    inp = R.inputs(c.name)
    srcs = [ops.Src3(_ndhwc(x, dt).to(DEV), *s[4:7]) for x, s in zip(inp.xs, c.srcs)]
    wp = ops.pack_conv3d_weight(inp.w.to(DEV), transposed=c.transposed, bf16=bf)
    gn = None
    if c.gn:
        gn = ops.GN(ops.gn_stats3d(srcs, c.dhw, c.gn), inp.gamma.to(DEV), inp.beta.to(DEV), c.gn, R.GN_EPS)
    B, oC, oD, oH, oW = c.out_shape
    out = Guarded((B, oD, oH, oW, oC), dt, _ndhwc(inp.prefill, dt).to(DEV) if c.partial else None)
    addend = _ndhwc(inp.addend, dt).to(DEV) if c.addend else None
    st = ops.new_stats(B, srcs[0].t) if c.stats else None
    routes = []
    real = nps_hip.lib.nps_conv3d_fwd

    def fwd(aref, stream):
        routes.append(R.route_of(aref._obj))
        return real(aref, stream)

    monkeypatch.setattr(nps_hip.lib, "nps_conv3d_fwd", fwd)
    monkeypatch.setattr(ops, "CONV3D_PACK", c.pack)
    nps_hip.lib.nps_conv3d_1x1_set_grid(c.grid)
    try:
        ops.conv3d(srcs, c.dhw, wp, inp.bias.to(DEV) if c.bias else None, c.Cout, c.K, stride=c.stride,
                   transposed=c.transposed, circ=c.circ, zpad=c.zpad, gn=gn, pre_act=c.pre_act, out=out.t,
                   out_os=2 if c.transposed else c.out_os, out_off=c.out_off, accumulate=c.accumulate, addend=addend,
                   act=c.act, out_stats=st)
        torch.cuda.synchronize()
    finally:
        nps_hip.lib.nps_conv3d_1x1_set_grid(0)
    return out, st, routes


@pytest.mark.parametrize("name,dtn", R.CONV_PARAMS)
def test_conv3d_row(name, dtn, monkeypatch):
    from nps_hip import ops
    c, dt = R.BY_NAME[name], R.DTYPES[dtn]
    out, st, routes = _run(c, dt, monkeypatch)
    assert routes == [c.route(dtn)]
    out.assert_guards()
    raw = _logical(out.t)
    got, ref = raw.double(), R.refs(name, dt)
    m = R.touched_mask(c)
    if c.partial:   # outside the window and at channels >= Cout: bit-unchanged
        pre = R.inputs(name).prefill.to(dt)
        assert torch.equal(_bits(raw[~m]), _bits(pre[~m])), "the launch wrote outside its window"
    gw, rw = R.window(c, got), R.window(c, ref)
    assert gw.numel() == int(m.sum())
    ratio = None
    if c.plain:
        ratio = ((gw - rw).abs() / R.bound(c, dt)).max().item()
    whole, worst, where = _slice_errors(gw, rw)
    print(f"ROW {name} {dtn} {routes[0]} bound-ratio {ratio if ratio is None else format(ratio, '.3f')} "
          f"rel-L2 {whole:.3e} worst-slice {worst:.3e} at {where}")
    if c.plain:
        assert ratio <= 1.0, "outside the elementwise bound"
    assert whole < R.TOL[dt] and worst < R.TOL[dt]
    if c.stats:     # the moments of the stored values (of the change, under accumulate)
        carried = ops._stats_sum([st], c.B, ops.new_stats(c.B, out.t, 1)).cpu()[:, 0]
        s1, s2 = gw.reshape(c.B, -1).sum(1), gw.reshape(c.B, -1).square().sum(1)
        if c.accumulate:
            old = R.window(c, R.inputs(name).prefill.to(dt).double()).reshape(c.B, -1)
            s1, s2 = s1 - old.sum(1), s2 - old.square().sum(1)
        # (tests/test_gpu_conv3d.py's tolerances: a plain conv3d_kernel epilogue; every other producer)
        plain = not (c.accumulate or c.addend or c.act or "1x1_kernel" in routes[0])
        tol = dict(rtol=1e-6, atol=1e-3) if plain else dict(rtol=1e-5, atol=1e-2)
        torch.testing.assert_close(carried[:, 0], s1, **tol)
        torch.testing.assert_close(carried[:, 1], s2, **tol)


# ------------------------------------------------------------------------------------ gn_stats3d / frame_pack3d
FRAME_PARAMS = [(c.name, dtn) for c in R.FRAME_CASES for dtn in R.DTYPES]


def _frame_srcs(c, dt):
    from nps_hip import ops
    xs, gamma, beta = R.frame_inputs(c.name)
    return [ops.Src3(_ndhwc(x, dt).to(DEV), *s[4:7]) for x, s in zip(xs, c.srcs)], gamma, beta


def _pack(c, dt, srcs, gn, pre_act):
    """nps_frame_pack3d into a guarded buffer: (B, C16, D, H, W) on the CPU in the storage dtype"""
    import nps_hip
    from nps_hip import ops
    a = ops._fill_frame3(nps_hip.Conv3dArgs(), srcs, c.dhw)
    ops._set_prologue(a, gn, pre_act)
    cpad = (c.Cin + 15) // 16 * 16
    out = Guarded((c.B,) + tuple(c.dhw) + (cpad,), dt)
    nps_hip.check(nps_hip.lib.nps_frame_pack3d(ctypes.byref(a), nps_hip.ptr(out.t), cpad, nps_hip.stream_ptr()),
                  "frame_pack3d")
    out.assert_guards()
    return _logical(out.t)


@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("name,dtn", FRAME_PARAMS)
def test_gn_stats3d_frame(name, dtn, groups):
    from nps_hip import ops
    c, dt = R.FRAME_BY_NAME[name], R.DTYPES[dtn]
    srcs, _, _ = _frame_srcs(c, dt)
    st = ops.gn_stats3d(srcs, c.dhw, groups).cpu()
    g = R.frame_of(c, dt).view(c.B, groups, c.Cin // groups, *c.dhw)
    torch.testing.assert_close(st[:, :, 0], g.sum((2, 3, 4, 5)), rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(st[:, :, 1], g.square().sum((2, 3, 4, 5)), rtol=1e-6, atol=1e-3)


@pytest.mark.parametrize("name,dtn", FRAME_PARAMS)
def test_frame_pack3d_without_prologue_is_the_frame(name, dtn):
    """pure concatenation, crop and channel padding: bit-exact, the pad channels exactly zero"""
    c, dt = R.FRAME_BY_NAME[name], R.DTYPES[dtn]
    srcs, _, _ = _frame_srcs(c, dt)
    p = _pack(c, dt, srcs, None, 0)
    xs, _, _ = R.frame_inputs(name)
    want = R.frame([(x.to(dt), s[4:7]) for x, s in zip(xs, c.srcs)], c.B, c.dhw)
    assert torch.equal(_bits(p[:, :c.Cin]), _bits(want))
    assert p.shape[1] % 16 == 0 and bool((_bits(p[:, c.Cin:]) == 0).all())


@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("name,dtn", FRAME_PARAMS)
def test_frame_pack3d_group_norm_gelu(name, dtn, groups):
    from nps_hip import ops
    c, dt = R.FRAME_BY_NAME[name], R.DTYPES[dtn]
    srcs, gamma, beta = _frame_srcs(c, dt)
    gn = ops.GN(ops.gn_stats3d(srcs, c.dhw, groups), gamma.to(DEV), beta.to(DEV), groups, R.GN_EPS)
    p = _pack(c, dt, srcs, gn, 1)
    want = R._rt(R.prologue(R.frame_of(c, dt), (groups, gamma, beta), 1), dt)
    assert bool((_bits(p[:, c.Cin:]) == 0).all())
    got = p[:, :c.Cin].double()
    tol = 1e-2 if dt == torch.bfloat16 else 1e-6
    worst = 0.0
    for dim in (2, 3, 4):   # every voxel slice
        for i in range(got.shape[dim]):
            worst = max(worst, rel_l2(got.select(dim, i), want.select(dim, i)))
    whole = rel_l2(got, want)
    print(f"PACK {name} {dtn} G{groups} rel-L2 {whole:.3e} worst-voxel-slice {worst:.3e}")
    assert whole < tol and worst < tol


# ------------------------------------------------------------------------------------ nps_conv3d_pack_weights
@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("Cout,Cin,K,transposed", R.PACK_CASES)
def test_conv3d_pack_weights_layout(Cout, Cin, K, transposed, dtn):
    """[phase][tile][kd][chunk][kh][kw][64][16] of include/nps.h built with torch indexing on the CPU: bit-exact in
    fp32, equal to the bf16 rounding of it in bf16; zero Cout / Cin tails; the 8-phase index rule; the grid-stride loop
    (the last case has more elements than the grid has threads)."""
    import nps_hip
    dt = R.DTYPES[dtn]
    bf = int(dt == torch.bfloat16)
    g = torch.Generator().manual_seed(1000 * Cout + Cin)
    w = torch.randn((Cin, Cout, 4, 4, 4) if transposed else (Cout, Cin, K, K, K), generator=g)
    want = R.pack_weight_reference(w, K, transposed).to(dt)
    nbytes = nps_hip.lib.nps_conv3d_packed_bytes(Cout, Cin, K, int(transposed), bf)
    assert nbytes == want.numel() * (2 if bf else 4)
    out = Guarded((want.numel(),), dt)
    wd = w.to(DEV)
    nps_hip.check(nps_hip.lib.nps_conv3d_pack_weights(nps_hip.ptr(wd), nps_hip.ptr(out.t), Cout, Cin, K,
                                                      int(transposed), bf, nps_hip.stream_ptr()), "conv3d_pack_weights")
    out.assert_guards()
    assert torch.equal(_bits(out.t.cpu()), _bits(want))
