"""The 3-D U-Net / U-FNO option matrix on the MI355X: every row of tests/unet3d_matrix.py as a whole network, in the
inference form (run3d: the fused launches, carried moments) and the autograd form (run_ad3d: the same kernels unfused
plus their backward kernels), against the fp64 oracle on the same parameters: y of both forms, dh, dvb and every
parameter gradient at the project's fp32 bar, rel-L2 < 1e-5 (grad_check.TOL; grad_check.grads_ok for the parameters).
The fp32 oracle itself sits 9.5e-8 ... 8.6e-7 from the fp64 one on these rows (test_unet3d_matrix_host.py).

The inference form is forward() under no_grad.  The autograd form of a U-FNO row is forward() in grad mode; a 3-D
UNetModern's forward() refuses grad mode (models.common.run_form, DESIGN.md "Deliberate deviations"), so a U-Net row
enters its autograd form where training does, at UNetModern.run_ad3d between the differentiable layout transposes.

bf16 storage (inference only): four rows run run3d on bf16 NDHWC inputs and are compared with this build's fp32 result
on the same row at the project's bar for it (tests/test_gpu_ufno3d.py BF16_TOL = 2e-2); the two geometries bf16 storage
refuses by design must raise NotImplementedError with their reason.

The test_routes_* tests pin WHICH launches a handful of the rows reach (frame_pack3d or not, carried moments or a
statistics pass, the kernel instantiation nps_conv3d_route names), so an eligibility change on the host cannot move the
matrix onto a fallback while the rows above stay green.
"""
import functools

import pytest
import torch

from conftest import rel_l2
import conv3d_ref
from grad_check import TOL, grads_ok
import unet3d_matrix as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_TOL = 2e-2   # tests/test_gpu_ufno3d.py::BF16_TOL


@functools.lru_cache(maxsize=None)
def _case(rid):
    """(module on the GPU, CPU inputs, fp64 reference) of a row, built once."""
    row = M.BY_ID[rid]
    m = M.build_module(row)
    h, vb, gy = M.inputs(row)
    ref = M.reference(row, m.state_dict(), h, vb, gy)
    # the host tests' stand-in state_dict is this module's: same keys, shapes and dtypes
    sig = lambda sd: {k: (tuple(v.shape), v.dtype) for k, v in sd.items()}  # noqa: E731
    assert sig(M.standin_state_dict(row)) == sig(m.state_dict())
    return m.to(DEV), (h, vb, gy), ref


def _infer(m, h, vb):
    with torch.no_grad():
        return m(h.to(DEV), variables_broadcast=vb.to(DEV) if vb is not None else None)


def _autograd(row, m, hd, vd):
    from models.common import ad_to_ncdhw, ad_to_ndhwc
    if M.is_ufno(row):
        return m(hd, variables_broadcast=vd)
    return ad_to_ncdhw(m.run_ad3d(ad_to_ndhwc(hd), ad_to_ndhwc(vd) if vd is not None else None))


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_forward_and_backward_vs_fp64_oracle(rid):
    row = M.BY_ID[rid]
    m, (h, vb, gy), ref = _case(rid)
    y = _infer(m, h, vb)
    hd = h.to(DEV).requires_grad_(True)
    vd = vb.to(DEV).requires_grad_(True) if vb is not None else None
    for p in m.parameters():
        p.grad = None
    y_ad = _autograd(row, m, hd, vd)
    y_ad.backward(gy.to(DEV))
    got = {k: p.grad for k, p in m.named_parameters()}
    e, e_ad, e_dh = rel_l2(y, ref.y), rel_l2(y_ad, ref.y), rel_l2(hd.grad, ref.dh)
    e_dvb = rel_l2(vd.grad, ref.dvb) if vb is not None else 0.0
    keys = list(ref.grads)
    assert all(got[k] is not None for k in keys)
    flat = lambda d: torch.cat([torch.view_as_real(d[k]).reshape(-1) if d[k].is_complex()  # noqa: E731
                                else d[k].reshape(-1) for k in keys]).cpu().double()
    e_par = (torch.linalg.vector_norm(flat(got) - flat(ref.grads)) / torch.linalg.vector_norm(flat(ref.grads))).item()
    print(f"{rid}: inference {e:.2e} autograd {e_ad:.2e} dh {e_dh:.2e} dvb {e_dvb:.2e} params {e_par:.2e}")
    for t in [y, y_ad, hd.grad] + ([vd.grad] if vd is not None else []) + list(got.values()):
        assert t is not None and torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()
    assert y.shape == ref.y.shape and y_ad.shape == ref.y.shape and y_ad.requires_grad and not y.requires_grad
    assert hd.grad.shape == ref.dh.shape and (vd is None or vd.grad.shape == ref.dvb.shape)
    assert e < TOL, "inference form"
    assert e_ad < TOL, "autograd form"
    assert e_dh < TOL and e_dvb < TOL
    grads_ok(ref.grads, got)


# ------------------------------------------------------------------------------------------------ bf16 storage
def _run3d_bf16(m, h, vb):
    from models.common import to_ncdhw, to_ndhwc
    from nps_hip import ops
    hb = ops.to_bf16(to_ndhwc(h.to(DEV)))
    vbb = ops.to_bf16(to_ndhwc(vb.to(DEV))) if vb is not None else None
    with torch.no_grad():
        return to_ncdhw(ops.to_f32(m.run3d(hb, vbb)))


@pytest.mark.parametrize("rid", [r.id for r in M.BF16_ROWS])
def test_row_bf16_storage_vs_fp32(rid):
    """run3d on bf16 NDHWC inputs (bf16 activations and packed weights, fp32 accumulation and GroupNorm statistics)
    against this build's fp32 inference result of the same row, as test_ufno3d_c5_volume_fp32_vs_oracle_and_bf16_vs_fp32
    does at the C5 volume."""
    m, (h, vb, _), ref = _case(rid)
    y32 = _infer(m, h, vb)
    yb = _run3d_bf16(m, h, vb)
    e32, err = rel_l2(y32, ref.y), rel_l2(yb.cpu(), y32.cpu())
    print(f"{rid}: bf16 storage vs fp32 rel-L2 {err:.2e} (fp32 vs the fp64 oracle {e32:.2e})")
    assert yb.shape == y32.shape and torch.isfinite(yb).all()
    assert e32 < TOL
    assert err < BF16_TOL


@pytest.mark.parametrize("rid", sorted(M.BF16_REFUSED))
def test_row_bf16_storage_refused_with_its_reason(rid):
    """bf16 storage refuses two geometries by design, by name: the zero border under a fused addend (UNetModern.run3d:
    the unfused add-then-activate is fp32) and the identity shortcut on a concatenation (ResidualBlock.run3d: the
    concatenation is materialised by the fp32 nps_frame3d_fwd)."""
    m, (h, vb, _), _ = _case(rid)
    with pytest.raises(NotImplementedError, match=M.BF16_REFUSED[rid]):
        _run3d_bf16(m, h, vb)


# ------------------------------------------------------------------------------------------------ routes
def _is_simple(srcs, frame_dhw, gn, pre_act):
    """ops.conv3d's `simple`: a single whole-frame source, C % 16 == 0 and no prologue."""
    s = srcs[0]
    return (len(srcs) == 1 and gn is None and not pre_act and tuple(s.t.shape[1:4]) == tuple(frame_dhw)
            and not (s.off_d or s.off_h or s.off_w) and s.t.shape[4] % 16 == 0)


class _Spy:
    """Records every ops.conv3d / ops.frame_pack3d / ops.frame3d / ops.gn_stats3d call of one inference forward, and
    for every nps_conv3d_fwd launch the kernel instantiation nps_conv3d_route names for the same arguments."""

    def __init__(self, monkeypatch):
        self.monkeypatch = monkeypatch
        self.convs, self.packs, self.frames, self.stats, self.routes = [], [], [], [], []

    def _patch(self, monkeypatch):
        from nps_hip import ops
        real_conv, real_pack, real_frame, real_stats = ops.conv3d, ops.frame_pack3d, ops.frame3d, ops.gn_stats3d
        real_fwd = ops.lib.nps_conv3d_fwd

        def conv3d(srcs, frame_dhw, wpack, bias, Cout, K, **kw):
            n0, r0 = len(self.packs), len(self.routes)
            rec = dict(K=K, Cout=Cout, C=tuple(s.t.shape[4] for s in srcs), stride=kw.get("stride", 1),
                       transposed=bool(kw.get("transposed", False)), gn=kw.get("gn"), pre_act=kw.get("pre_act", 0),
                       simple=_is_simple(srcs, frame_dhw, kw.get("gn"), kw.get("pre_act", 0)),
                       accumulate=bool(kw.get("accumulate", False)), out_stats=kw.get("out_stats") is not None,
                       bf16=srcs[0].t.dtype == torch.bfloat16)
            self.convs.append(rec)
            out = real_conv(srcs, frame_dhw, wpack, bias, Cout, K, **kw)
            rec["packed"] = len(self.packs) > n0   # the launch was fed by nps_frame_pack3d
            assert len(self.routes) == r0 + 1      # one nps_conv3d_fwd per ops.conv3d (the 8 phases too: one launch)
            rec["route"] = self.routes[-1]
            return out

        def frame_pack3d(srcs, frame_dhw, gn=None, pre_act=0):
            out = real_pack(srcs, frame_dhw, gn, pre_act)
            self.packs.append(dict(C=tuple(s.t.shape[4] for s in srcs), gn=gn, pre_act=pre_act, Cpad=out.shape[4]))
            return out

        def frame3d(srcs, frame_dhw, gn=None, pre_act=0):
            self.frames.append(dict(C=tuple(s.t.shape[4] for s in srcs), gn=gn, pre_act=pre_act))
            return real_frame(srcs, frame_dhw, gn, pre_act)

        def gn_stats3d(srcs, frame_dhw, groups):
            self.stats.append(dict(C=tuple(s.t.shape[4] for s in srcs), groups=groups,
                                   whole=len(srcs) == 1 and tuple(srcs[0].t.shape[1:4]) == tuple(frame_dhw)))
            return real_stats(srcs, frame_dhw, groups)

        def fwd(ref, stream):
            self.routes.append(conv3d_ref.route_of(ref._obj))
            return real_fwd(ref, stream)

        monkeypatch.setattr(ops, "conv3d", conv3d)
        monkeypatch.setattr(ops, "frame_pack3d", frame_pack3d)
        monkeypatch.setattr(ops, "frame3d", frame3d)
        monkeypatch.setattr(ops, "gn_stats3d", gn_stats3d)
        monkeypatch.setattr(ops.lib, "nps_conv3d_fwd", fwd)

    def run(self, rid, bf16=False):
        m, (h, vb, _), ref = _case(rid)
        with self.monkeypatch.context() as mp:   # (patched for this forward only: a test may spy on several rows)
            self._patch(mp)
            y = _run3d_bf16(m, h, vb) if bf16 else _infer(m, h, vb)
            torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        if not bf16:
            assert rel_l2(y, ref.y) < TOL
        self.check_packing()
        return self

    def check_packing(self):
        """ops.conv3d: `if CONV3D_PACK and K > 1 and not simple` the frame is materialised by nps_frame_pack3d first.
        No frame_pack3d before a conv that is simple (or pointwise); one before every K > 1 conv that is not; and what
        the packed conv launches is the SIMPLE instantiation (the pack pads the channels to a multiple of 16)."""
        assert self.convs and len(self.packs) == sum(c["packed"] for c in self.convs)
        for c in self.convs:
            assert c["packed"] == (c["K"] > 1 and not c["simple"]), c
            if c["K"] > 1:
                assert ",SIMPLE," in c["route"], c
        assert all(p["Cpad"] % 16 == 0 and 0 <= p["Cpad"] - sum(p["C"]) < 16 for p in self.packs)

    def of(self, **want):
        return [c for c in self.convs if all(c[k] == v for k, v in want.items())]




def _structure(row):
    """(blocks, downsamples, upsamples) of one U-Net of the row in walk order, from oracle.functional.unet_structure:
    blocks = [(source channels of the ResidualBlock's frame, Cout)], the frame being (h, vb) on the way down,
    (h, skip, vb) on the way up; down / upsamples = their channel counts."""
    import math
    from oracle import functional as Fo
    c = row.case
    down, _, up = Fo.unet_structure(c.hidden, c.ch_mults, c.n_blocks, c.n_cond)
    vb = (c.n_cond,) if c.n_cond else ()
    top = c.hidden * math.prod(c.ch_mults)
    blocks = [((m[1] - c.n_cond,) + vb, m[2]) for m in down if m[0] == "down"]
    blocks += [((top,) + vb, top), ((top,), top)]
    blocks += [((m[1] - c.n_cond, m[2]) + vb, m[2]) for m in up if m[0] == "up"]
    return blocks, [m[1] for m in down if m[0] == "downsample"], [m[1] for m in up if m[0] == "upsample"]


def _pointwise(row):
    """The 1x1x1 convs of one U-Net in launch order: a shortcut wherever a block's frame has another channel count
    than its output, then the final conv when use1x1."""
    blocks, _, _ = _structure(row)
    return [b for b in blocks if sum(b[0]) != b[1]] + ([((row.case.hidden,), row.case.hidden)] * row.case.use1x1)


def _pad16(n):
    return (n + 15) // 16 * 16


def _check_structure(s, row, unets=1):
    """What only the host decides, for any row (ops.conv3d `simple`, CONV3D_PACK): every ResidualBlock conv carries the
    GELU prologue (pre_act), so none is simple and all are fed by nps_frame_pack3d (conv1 with the block's frame
    padded to a multiple of 16 channels, GroupNorm(1) prologue on norm=True rows); a Downsample / Upsample of C
    channels is simple exactly when C % 16 == 0, one transposed launch per Upsample; the 1x1x1 convs are never
    packed."""
    c = row.case
    blocks, downs, ups = _structure(row)
    k3 = s.of(K=3, stride=1)
    assert len(k3) == unets * (2 * len(blocks) + (not c.use1x1))
    assert all(x["packed"] and x["pre_act"] and (x["gn"] is not None) == c.norm for x in k3)
    assert all(x["gn"].groups == 1 for x in k3[:2 * len(blocks)] if c.norm)
    conv1 = [x for x in k3 if not x["accumulate"]][:len(blocks)]
    assert [x["C"] for x in conv1] == [b[0] for b in blocks]
    want = [((C,), C % 16 != 0) for d in downs for C in [d] + ([c.n_cond] if c.n_cond else [])] * unets
    assert [(x["C"], x["packed"]) for x in s.of(K=3, stride=2)] == want
    assert [(x["K"], x["C"], x["packed"]) for x in s.of(transposed=True)] == [
        (2, (C,), C % 16 != 0) for C in ups] * unets
    assert all(x["out_stats"] for x in s.of(transposed=True))
    k1 = s.of(K=1)
    assert [(x["C"], x["Cout"]) for x in k1] == _pointwise(row) * unets and not any(x["packed"] for x in k1)
    packs = {p["C"]: p["Cpad"] for p in s.packs}
    assert all(packs[b[0]] == _pad16(sum(b[0])) for b in blocks)
    # conv2 accumulates into the shortcut's output (or the identity's copy) and hands on the block output's moments
    acc = s.of(accumulate=True)
    assert len(acc) == unets * len(blocks) and all(x["K"] == 3 and x["out_stats"] == c.norm for x in acc)


def _check_moments(s, row, unets=1, inputs_with_moments=0):
    """norm=True rows, ops.group_norm_stats3d with ops.CARRY3D: a GroupNorm(1) frame whose sources carry moments takes
    their sum, no nps_gn_stats3d pass.  Every producer inside the network hands its moments on (Downsample, Upsample,
    the ResidualBlocks: out_stats), so the only GroupNorm(1) passes are over tensors no conv of the walk produced with
    out_stats: the network input h, once, and vb at each level, once (Downsample.run3d runs vb's conv without out_stats;
    source_stats3d keeps the result on the tensor for the later frames).  Each is a single whole source.  The final
    GroupNorm(8, hidden) has no carried form: one pass per U-Net."""
    from nps_hip import ops
    c = row.case
    assert ops.CARRY3D and c.norm
    g1 = [x for x in s.stats if x["groups"] == 1]
    assert all(x["whole"] and len(x["C"]) == 1 for x in g1), g1
    n_vb = len(c.ch_mults) if c.n_cond > 0 else 0
    # (a U-FNO's conditioning is the same tensor in every block: its level-0 moments are taken once; a later block's
    # input carries the moments the previous block's final conv added)
    want = unets * (1 + n_vb) - inputs_with_moments - (unets - 1) * min(n_vb, 1)
    assert len(g1) == want, (len(g1), want, g1)
    assert [(x["groups"], x["C"]) for x in s.stats if x["groups"] != 1] == [(8, (c.hidden,))] * unets


def test_routes_aligned_hidden16(monkeypatch):
    """hidden 16, ch_mults (1, 2), n_cond 4, norm, use1x1, fp32: 8 ResidualBlocks, so 16 packed 3x3x3 convs plus vb's
    Downsample (C = 4) = 17 nps_frame_pack3d; h's Downsample (C = 16) and the Upsample are simple.  The packed K > 1
    convs launch the SIMPLE instantiations; the 1x1x1 convs (7 shortcuts over 2 or 3 sources, the final conv with its
    GroupNorm(8) prologue) launch conv3d_kernel<f32,1,1,8,GENERAL,REG>: the streaming 1x1x1 kernel is bf16-only
    (conv3d.hip c3d_1x1_eligible begins `if (!a.bf16 ...) return false`)."""
    R = conv3d_ref.R
    row = M.BF16_ROWS[0]
    s = _Spy(monkeypatch).run(row.id)
    _check_structure(s, row)
    assert len(s.packs) == 17 and s.frames == []
    assert {x["route"] for x in s.of(K=3, stride=1)} == {R("f32", 3, 1, True)}
    assert [(x["C"], x["packed"], x["route"]) for x in s.of(K=3, stride=2)] == [
        ((16,), False, R("f32", 3, 2, True)), ((4,), True, R("f32", 3, 2, True))]
    assert [(x["C"], x["packed"], x["route"]) for x in s.of(transposed=True)] == [((16,), False, R("f32", 2, 1, True))]
    k1 = s.of(K=1)
    assert [x["C"] for x in k1] == [(16, 4), (16, 4), (32, 4), (32, 32, 4), (32, 16, 4), (16, 16, 4), (16, 16, 4),
                                    (16,)]
    assert all(x["route"] == R("f32", 1, 1, False) for x in k1)
    assert k1[-1]["gn"].groups == 8 and all(x["gn"] is None and not x["pre_act"] for x in k1[:-1])
    _check_moments(s, row)
    assert [x["C"] for x in s.stats] == [(16,), (4,), (4,), (16,)]


def test_routes_no_norm_no_cond_hidden16(monkeypatch):
    """norm=False, n_cond 0, use1x1=False: no GroupNorm, so no statistics pass at all; the ResidualBlock convs and the
    3x3x3 final conv still carry the GELU prologue and are packed; the level-1 DownBlock(16, 32) shortcut is a
    single-source, 16-channel, prologue-free 1x1x1 conv: the one SIMPLE K = 1 launch."""
    R = conv3d_ref.R
    row = M.find(hidden=16, ch_mults=(1, 2), norm=False, use1x1=False, n_cond=0, dhw=(11, 12, 13))
    s = _Spy(monkeypatch).run(row.id)
    _check_structure(s, row)
    assert s.stats == [] and s.frames == []
    assert [(x["C"], x["route"]) for x in s.of(K=1)] == [
        ((16,), R("f32", 1, 1, True)), ((32, 32), R("f32", 1, 1, False)), ((32, 16), R("f32", 1, 1, False)),
        ((16, 16), R("f32", 1, 1, False)), ((16, 16), R("f32", 1, 1, False))]


def test_routes_unaligned_hidden8_and_hidden24(monkeypatch):
    """hidden 8 / n_cond 2 (no channel count a multiple of 16) and hidden 24 / n_cond 4 (sources off a 16-channel
    boundary): every K > 1 conv is packed, h's Downsample and the Upsample (8 / 24 channels) included, and the pack
    pads the 10-, 18-, 26- and 34-channel frames (hidden 8) and the 28-, 52-, 76- and 100-channel ones (hidden 24) up
    to the next multiple of 16."""
    row = M.find(hidden=8)
    s = _Spy(monkeypatch).run(row.id)
    _check_structure(s, row)
    assert [(x["C"], x["packed"]) for x in s.of(K=3, stride=2) + s.of(transposed=True)] == [
        ((8,), True), ((2,), True), ((8,), True)]
    assert {C: n for C, n in {p["C"]: p["Cpad"] for p in s.packs}.items() if len(C) > 1} == {
        (8, 2): 16, (16, 2): 32, (16, 16, 2): 48, (16, 8, 2): 32, (8, 8, 2): 32}
    _check_moments(s, row)
    row = M.find(hidden=24)
    s = _Spy(monkeypatch).run(row.id)
    _check_structure(s, row)
    assert [(x["C"], x["packed"]) for x in s.of(K=3, stride=2) + s.of(transposed=True)] == [
        ((24,), True), ((4,), True), ((24,), True)]
    assert {C: n for C, n in {p["C"]: p["Cpad"] for p in s.packs}.items() if len(C) > 1} == {
        (24, 4): 32, (48, 4): 64, (48, 48, 4): 112, (48, 24, 4): 80, (24, 24, 4): 64}
    _check_moments(s, row)


def test_routes_identity_on_a_concatenation(monkeypatch):
    """hidden 16, n_cond 16, ch_mults (1, 2): the level-1 DownBlock is ResidualBlock(32, 32) and its identity
    shortcut adds cat(h, vb).  ResidualBlock.run3d materialises the concatenation exactly once with a plain
    nps_frame3d_fwd (no GroupNorm, no activation; conv1's own frame is a separate nps_frame_pack3d with the prologue),
    conv2 accumulates into it, and the block output carries the sum of the sources' moments plus conv2's change: the
    middle block's norm1 takes no statistics pass (_check_moments counts them)."""
    row = M.IDENT_CAT_ROW
    s = _Spy(monkeypatch).run(row.id)
    _check_structure(s, row)
    assert ((16, 16), 32) in _structure(row)[0] and ((16, 16), 32) not in _pointwise(row)
    assert [(f["C"], f["gn"], f["pre_act"]) for f in s.frames] == [((16, 16), None, 0)]
    _check_moments(s, row)
    assert [x["C"] for x in s.stats] == [(16,), (16,), (16,), (16,)]   # h, vb at two levels, the final GroupNorm(8)
    # the U-FNO of the same configuration: block 1's output (the final conv's out_stats) feeds block 2's norm1 frames
    s = _Spy(monkeypatch).run(M.IDENT_CAT_UFNO_ROW.id)
    _check_structure(s, M.IDENT_CAT_UFNO_ROW, unets=2)
    assert [f["C"] for f in s.frames] == [(16, 16)] * 2
    _check_moments(s, M.IDENT_CAT_UFNO_ROW, unets=2, inputs_with_moments=1)


def test_routes_three_levels(monkeypatch):
    """ch_mults (1, 1, 2): two Downsamples of h (simple) and of vb (packed), one transposed launch per Upsample, and
    vb's moments taken once per level."""
    s = _Spy(monkeypatch).run(M.DEPTH_ROW.id)
    _check_structure(s, M.DEPTH_ROW)
    assert [(x["C"], x["packed"]) for x in s.of(K=3, stride=2)] == [((16,), False), ((4,), True)] * 2
    assert [(x["C"], x["packed"]) for x in s.of(transposed=True)] == [((16,), False)] * 2
    _check_moments(s, M.DEPTH_ROW)
    assert len([x for x in s.stats if x["C"] == (4,)]) == 3


def test_routes_wide_cout192_and_cout256(monkeypatch):
    """hidden 48 and 64 with ch_mults (2, 2) in fp32: the Cout-192 / Cout-256 3x3x3 convs (packed: SIMPLE) take three
    / four 64-channel tiles of conv3d_kernel<f32,3,1,8,SIMPLE,REG> (conv3d.hip launch: grid.y = ntile), and the 1x1x1
    shortcuts to 192 / 256 channels over (96, 4), (192, 4), (192, 192, 4) / (128, 4), (256, 4), (256, 256, 4) sources,
    Cin up to 516, stay on conv3d_kernel<f32,1,1,8,GENERAL,REG> and still hand on their moments."""
    R = conv3d_ref.R
    for row, wide in ((M.WIDE192_ROW, 192), (M.WIDE256_ROW, 256)):
        s = _Spy(monkeypatch).run(row.id)
        _check_structure(s, row)
        k3 = [x for x in s.of(K=3, stride=1) if x["Cout"] == wide]
        assert len(k3) == 2 * 4 and all(x["route"] == R("f32", 3, 1, True) for x in k3)  # down.2, middle x 2, up.0
        sc = [x for x in s.of(K=1) if x["Cout"] == wide]
        assert [x["C"] for x in sc] == [(wide // 2, 4), (wide, 4), (wide, wide, 4)]
        assert all(x["route"] == R("f32", 1, 1, False) and x["out_stats"] for x in sc)
        assert max(sum(x["C"]) for x in s.convs) == 2 * wide + 4
        _check_moments(s, row)


def _bf16_pointwise_route(C, Cout, pro):
    """conv3d.hip for a bf16 1x1x1 conv.  c3d_1x1_eligible: Cout <= 128, Cin <= 256, Cout % 4 == 0, every source
    C % 4 == 0 (C % 8 == 0 unless last), at most two sources -> conv3d_1x1_kernel<NCB,NCH,PRO|PLAIN> (dispatch_1x1:
    NCB 4 when Cout > 64; NCH 5 / 9 / 16 for up to 5 / 9 / 16 chunks of 16 input channels).  Else dispatch<bf16>: the
    streaming general kernel REG_O4 unless the frame is simple."""
    cin = sum(C)
    if (Cout <= 128 and cin <= 256 and Cout % 4 == 0 and len(C) <= 2 and all(c % 4 == 0 for c in C)
            and all(c % 8 == 0 for c in C[:-1])):
        nchunk = (cin + 15) // 16
        return conv3d_ref.R1(4 if Cout > 64 else 2, 5 if nchunk <= 5 else 9 if nchunk <= 9 else 16, pro)
    simple = len(C) == 1 and cin % 16 == 0 and not pro
    return conv3d_ref.R("bf16", 1, 1, simple, "REG" if simple else "REG_O4")


def test_routes_bf16_streaming_1x1x1_and_the_general_kernel_past_cout128(monkeypatch):
    """bf16 storage on three rows: the streaming 1x1x1 kernel where c3d_1x1_eligible admits it (two-source shortcuts up
    to Cout 128, the final conv with its GroupNorm(8) prologue: PRO), the general kernel
    conv3d_kernel<bf16,1,1,8,GENERAL,REG_O4> for three-source frames and above Cout 128 (hidden 48: the (96, 4) and
    (192, 4) shortcuts to 192 channels).  The packed / simple K > 1 convs take the LDS-DMA forms (dispatch: DMA for
    K = 3, DMA_O4 for the transposed conv's K = 2)."""
    R, R1 = conv3d_ref.R, conv3d_ref.R1
    gen = R("bf16", 1, 1, False, "REG_O4")
    for row in (M.BF16_ROWS[0], M.WIDE192_ROW, M.C5_ROW):
        s = _Spy(monkeypatch).run(row.id, bf16=True)
        assert all(x["bf16"] for x in s.convs)
        _check_structure(s, row)
        pw = _pointwise(row)
        want = [_bf16_pointwise_route(C, Cout, pro=(i == len(pw) - 1)) for i, (C, Cout) in enumerate(pw)]
        assert [x["route"] for x in s.of(K=1)] == want
        assert {x["route"] for x in s.of(K=3, stride=1)} == {R("bf16", 3, 1, True, "DMA")}
        assert {x["route"] for x in s.of(K=3, stride=2)} == {R("bf16", 3, 2, True, "DMA")}
        assert {x["route"] for x in s.of(transposed=True)} == {R("bf16", 2, 1, True, "DMA_O4")}
        if row is M.BF16_ROWS[0]:    # hidden 16, n_cond 4
            assert want == [R1(2, 5, False)] * 3 + [gen] * 4 + [R1(2, 5, True)]
        elif row is M.WIDE192_ROW:   # (48, 4) -> 96 streams; (96, 4) -> 192 and (192, 4) -> 192 are past Cout 128
            assert want == [R1(4, 5, False)] + [gen] * 6 + [R1(2, 5, True)]
        else:                        # C5's structure: three (64, 4) and four (64, 64, 4) shortcuts, the final conv
            assert want == [R1(2, 5, False)] * 3 + [gen] * 4 + [R1(2, 5, True)]
