"""The 2-D U-Net / U-FNO option matrix on the MI355X: every row of tests/unet2d_matrix.py as a whole network, in the
inference form (the fused launches) and the autograd form (the same kernels unfused plus their backward kernels),
against the fp64 oracle on the same parameters: y of both forms, dh, dvb and every parameter gradient at the
project's fp32 bar, rel-L2 < 1e-5 (BASELINE.json; grad_check.grads_ok for the parameters).  The fp32 oracle itself
sits 4.7e-8 ... 7.3e-7 from the fp64 one on these rows (test_unet2d_matrix_host.py), so the bar leaves > 10x.

The test_routes_* tests pin WHICH launches a handful of the rows reach (fused prologue / frame_pack, space-to-depth view /
copy / generic stride-2 conv, merged transposed-conv phases, the wide tile, carried moments), so an eligibility
change on the host cannot move the matrix onto a fallback while the rows above stay green.
"""
import functools

import pytest
import torch

from conftest import rel_l2
from grad_check import TOL, grads_ok
import unet2d_matrix as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _call(m, h, vb):
    return m(h, variables_broadcast=vb)


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_forward_and_backward_vs_fp64_oracle(rid):
    m, (h, vb, gy), ref = _case(rid)
    with torch.no_grad():
        y = _call(m, h.to(DEV), vb.to(DEV) if vb is not None else None)
    hd = h.to(DEV).requires_grad_(True)
    vd = vb.to(DEV).requires_grad_(True) if vb is not None else None
    for p in m.parameters():
        p.grad = None
    y_ad = _call(m, hd, vd)
    y_ad.backward(gy.to(DEV))
    got = {k: p.grad for k, p in m.named_parameters()}
    e, e_ad, e_dh = rel_l2(y, ref.y), rel_l2(y_ad, ref.y), rel_l2(hd.grad, ref.dh)
    e_dvb = rel_l2(vd.grad, ref.dvb) if vb is not None else 0.0
    keys = list(ref.grads)
    flat = lambda d: torch.cat([torch.view_as_real(d[k]).reshape(-1) if d[k].is_complex()  # noqa: E731
                                else d[k].reshape(-1) for k in keys]).cpu().double()
    e_par = (torch.linalg.vector_norm(flat(got) - flat(ref.grads)) / torch.linalg.vector_norm(flat(ref.grads))).item()
    print(f"{rid}: inference {e:.2e} autograd {e_ad:.2e} dh {e_dh:.2e} dvb {e_dvb:.2e} params {e_par:.2e}")
    for t in [y, y_ad, hd.grad] + ([vd.grad] if vd is not None else []) + list(got.values()):
        assert t is not None and torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()
    assert y.shape == ref.y.shape and y_ad.requires_grad
    assert e < TOL, "inference form"
    assert e_ad < TOL, "autograd form"
    assert e_dh < TOL and e_dvb < TOL
    grads_ok(ref.grads, got)


# ------------------------------------------------------------------------------------------------ routes
class _Spy:
    """Records every ops.conv2d / ops.frame_pack / ops.space_to_depth call and every nps_conv2d_plan result of one
    inference forward."""

    def __init__(self, monkeypatch):
        from nps_hip import ops
        self.convs, self.packs, self.s2d, self.plans = [], [], [], []
        real_conv, real_pack, real_s2d, real_plan = ops.conv2d, ops.frame_pack, ops.space_to_depth, ops.lib.nps_conv2d_plan

        def conv2d(srcs, frame_hw, wpack, bias, Cout, KH, KW, **kw):
            n0 = len(self.packs)
            rec = dict(K=KH, Cout=Cout, C=tuple(s.t.shape[3] for s in srcs), stride=kw.get("stride", 1),
                       gn=kw.get("gn"), pre_act=kw.get("pre_act", 0), s2d_pad=kw.get("s2d_pad"),
                       phases=kw.get("phases", 1), out_os=kw.get("out_os", 1), out_stats=kw.get("out_stats"),
                       addends=len(kw.get("addends", ())), act=kw.get("act", 0))
            self.convs.append(rec)
            out = real_conv(srcs, frame_hw, wpack, bias, Cout, KH, KW, **kw)
            rec["packed"] = len(self.packs) > n0   # the launch was fed by nps_frame_pack
            st = rec["out_stats"]
            rec["moments"] = st is not None and not getattr(st, "_nps_incomplete", False)
            return out

        def frame_pack(srcs, frame_hw, gn=None, pre_act=0, pad4=False):
            self.packs.append(dict(C=tuple(s.t.shape[3] for s in srcs), gn=gn, pre_act=pre_act, pad4=pad4))
            return real_pack(srcs, frame_hw, gn, pre_act, pad4=pad4)

        def space_to_depth(x, *a, **k):
            self.s2d.append(x.shape[3])
            return real_s2d(x, *a, **k)

        def plan(ref):
            r = real_plan(ref)
            a = ref._obj
            self.plans.append(dict(K=a.KH, Cout=a.Cout, Cin=a.Cin, tile=a.TH * a.TW, precision=a.precision,
                                   stride=a.stride))
            return r

        monkeypatch.setattr(ops, "conv2d", conv2d)
        monkeypatch.setattr(ops, "frame_pack", frame_pack)
        monkeypatch.setattr(ops, "space_to_depth", space_to_depth)
        monkeypatch.setattr(ops.lib, "nps_conv2d_plan", plan)

    def run(self, rid):
        from nps_hip import ops
        m, (h, vb, _), ref = _case(rid)
        ops.conv_probe = []
        try:
            with torch.no_grad():
                y = _call(m, h.to(DEV), vb.to(DEV) if vb is not None else None)
            torch.cuda.synchronize()
            self.classes = [p[3][0] for p in ops.conv_probe]  # "x3f16" | "f32" per launch, in call order
        finally:
            ops.conv_probe = None
        assert len(self.classes) == len(self.convs)
        assert rel_l2(y, ref.y) < TOL
        return self

    def fused(self, K):
        """Launches of a K x K conv whose GroupNorm prologue was handed to the kernel."""
        return [c for c in self.convs if c["K"] == K and c["gn"] is not None and not c["packed"]]


def _x3_only():
    from nps_hip import ops
    if ops.CONV_PRECISION != ops.PREC_X3F16:
        pytest.skip("the routes pinned here are the split-fp16 ones")


def test_routes_aligned_hidden16(monkeypatch):
    """hidden 16, ch_mults [1, 2], n_cond 4, norm, use1x1, 'ones', (21, 18).  Every frame is (16 | 32, [16 | 32,] 4)
    channels: each C % 4 == 0 and each source starts on a multiple of 16 (conv2d_common.hpp x3_sources_aligned), so
    no frame is materialised for alignment."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=16, ch_mults=(1, 2), padding_mode="ones", norm=True, use1x1=True, n_cond=4,
                                     hw=(21, 18)).id)
    # conv2d.hip x3_eligible: a 3x3 GroupNorm(1) prologue fuses when Cin % 4 == 0 (ops.conv2d `fused`): conv1 and
    # conv2 of the 2 down, 2 middle and 4 up ResidualBlocks (Cin 20, 36, 68, 52, 16, 32)
    assert all(c["gn"].groups == 1 for c in s.fused(3)) and len(s.fused(3)) == 16
    # ... but the final conv's GroupNorm(8, 16) has 2 channels per group: x3_eligible needs (Cin / groups) % 4 == 0,
    # so that ONE launch is fed by nps_frame_pack (hidden 32 below fuses it); no other frame_pack anywhere
    assert len(s.packs) == 1 and s.packs[0]["gn"].groups == 8 and s.packs[0]["C"] == (16,)
    final = s.convs[-1]
    assert final["K"] == 1 and final["packed"] and final["moments"]
    # Conv2d.run (models/common.py): the Downsample of h (C = 16, C % 16 == 0) reads the space-to-depth view
    # (s2d_pad = the conv's zero padding, 1); vb's (C = 4: C % 4 == 0 only) runs over a space_to_depth copy
    view = [c for c in s.convs if c["s2d_pad"] is not None]
    assert [(c["s2d_pad"], c["K"], c["C"]) for c in view] == [(1, 2, (16,))]
    assert s.s2d == [4] and [c["C"] for c in s.convs if c["K"] == 2 and c["s2d_pad"] is None
                             and c["phases"] == 1] == [(16,)]  # (the copy: 4 x 4 channels)
    assert not any(c["stride"] != 1 for c in s.convs)
    # ConvTranspose2d.run: one merged 4-phase launch per Upsample (one Upsample here), no per-phase launches
    assert [c["phases"] for c in s.convs if c["out_os"] == 2] == [4]
    # every launch is split-fp16, and every out_stats buffer handed to a conv came back complete (ops.conv2d: split-fp16,
    # Cout % 4 == 0, 1x1 only without accumulate and Cout <= 192)
    assert set(s.classes) == {"x3f16"}
    assert all(c["moments"] for c in s.convs if c["out_stats"] is not None)


def test_routes_aligned_hidden32(monkeypatch):
    """hidden 32, ch_mults [2, 1], two blocks per level, n_cond 4: frames of (32 | 64, [32 | 64,] 4) channels, all
    aligned; GroupNorm(8, 32) has 4 channels per group, so the final 1x1 conv (Cout 32 <= 192: ops.conv2d `fused`)
    takes its prologue in the kernel too: no frame_pack at all."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=32, ch_mults=(2, 1), padding_mode="ones", n_cond=4).id)
    assert s.packs == []
    assert [(c["gn"].groups, c["Cout"]) for c in s.fused(1)] == [(8, 32)]
    assert len(s.fused(3)) == 2 * 12  # conv1 + conv2 of 4 down, 2 middle and 6 up ResidualBlocks
    assert [c["s2d_pad"] for c in s.convs if c["s2d_pad"] is not None] == [1] and s.s2d == [4]
    assert set(s.classes) == {"x3f16"}


def test_routes_unaligned_hidden8(monkeypatch):
    """hidden 8, n_cond 2, two blocks per level: vb has C = 2 (C % 4 != 0), so every frame that holds it fails
    x3_sources_aligned and is materialised by nps_frame_pack with pad4 — its conv1 AND its 1x1 shortcut (ops.conv2d:
    `not aligned`).  A single 8- or 16-channel source is aligned and GroupNorm(1) fuses there (conv2, middle.res2);
    the final GroupNorm(8, 8) (1 channel per group) is packed."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=8, padding_mode="ones").id)
    multi = [c for c in s.convs if len(c["C"]) > 1]
    assert len(multi) == 2 * 11  # conv1 + the 1x1 shortcut of the 4 down blocks, middle.res1 and the 6 up blocks
    assert all(c["packed"] for c in multi)
    assert all(p["pad4"] for p in s.packs)
    assert s.convs[-1]["K"] == 1 and s.convs[-1]["packed"] and s.packs[-1]["gn"].groups == 8
    single = [c for c in s.convs if c["K"] == 3 and len(c["C"]) == 1 and c["gn"] is not None]
    assert single and not any(c["packed"] for c in single)
    # Conv2d.run: h (C = 8: C % 4 == 0, C % 16 != 0) -> the space-to-depth copy; vb (C = 2) -> the generic stride-2
    # 3x3 conv, which no split-fp16 kernel takes (x3_eligible: stride 1 only)
    assert not any(c["s2d_pad"] is not None for c in s.convs) and s.s2d == [8]
    s2 = [(c["C"], cls) for c, cls in zip(s.convs, s.classes) if c["stride"] == 2]
    assert s2 == [((2,), "f32")]


def test_routes_off_boundary_hidden24(monkeypatch):
    """hidden 24, ch_mults [1, 2], n_cond 4: every C % 4 == 0, but a source that follows 24 or 72 channels starts off
    a 16-channel boundary (x3_sources_aligned): the up-block frames (48, 24, 4) and (24, 24, 4) are packed with pad4,
    the frame (48, 48, 4) (sources at 0, 48, 96) is not."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=24, padding_mode="ones").id)
    up = {c["C"]: c["packed"] for c in s.convs if len(c["C"]) == 3 and c["K"] == 3}
    assert up == {(48, 48, 4): False, (48, 24, 4): True, (24, 24, 4): True}
    assert all(c["packed"] for c in s.convs if c["C"] == (24, 4))        # down.0 / down.2... frames: vb starts at 24
    assert not any(c["packed"] for c in s.convs if c["C"] == (48, 4))    # middle.res1: vb starts at 48
    assert all(p["pad4"] for p in s.packs)
    assert set(s.classes) == {"x3f16"}


def test_routes_wide_tile_hidden48(monkeypatch):
    """hidden 48, ch_mults [2, 2]: the Cout-192 3x3 convs (down.2, the middle block, up.0) are planned on the wide 192-channel x 128-pixel tile (conv2d_common.hpp x3_wide_eligible: 2x2 / 3x3,
    128 < Cout <= 192, Cout % 32 == 0; conv2d.hip nps_conv2d_plan), Cout 96 on the 64-channel tiles; the Cout-192 1x1
    shortcuts are at the limit up to which the 1x1 kernel takes the moments (ops.conv2d x1_ok)."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=48, padding_mode="ones", use1x1=True).id)
    x3 = [p for p in s.plans if p["precision"] == 1 and p["stride"] == 1]
    wide = [p for p in x3 if p["K"] == 3 and p["Cout"] == 192]
    assert len(wide) >= 6 and all(p["tile"] == 128 for p in wide)
    assert all(p["tile"] != 128 for p in x3 if p["K"] in (2, 3) and p["Cout"] <= 128)
    sc = [c for c in s.convs if c["K"] == 1 and c["Cout"] == 192]
    assert sc and all(c["gn"] is None and not c["pre_act"] and c["moments"] for c in sc)


def test_routes_past_192_hidden64(monkeypatch):
    """hidden 64, ch_mults [2, 2]: Cout 256 > 192.  The 1x1 shortcuts to 256 channels carry no prologue (a shortcut
    reads the raw frame) and are past the 1x1 kernel's fused-epilogue limit: their moments buffer comes back
    incomplete (ops.conv2d x1_ok: Cout <= 192) and the block's norm falls back to a statistics pass; no Cout-256
    conv is planned on the wide tile (x3_wide_eligible: Cout <= 192)."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=64, padding_mode="ones").id)
    sc = [c for c in s.convs if c["K"] == 1 and c["Cout"] == 256]
    assert sc and all(c["gn"] is None and not c["pre_act"] and not c["packed"] for c in sc)
    assert all(c["out_stats"] is not None and not c["moments"] for c in sc)
    assert all(p["tile"] != 128 for p in s.plans if p["Cout"] == 256)
    assert [(c["gn"].groups, c["Cout"]) for c in s.fused(1)] == [(8, 64)]  # the final conv: 8 channels per group


def test_routes_vb_view_and_identity_on_a_concatenation_hidden16_cond16(monkeypatch):
    """hidden 16, n_cond 16, ch_mults [1, 2, 2]: vb has 16 channels, so both Downsamples read h AND vb through the
    space-to-depth view (Conv2d.run: C % 16 == 0) and no space_to_depth copy is made; every frame is aligned.  The
    level-1 DownBlock is ResidualBlock(32, 32): its identity shortcut adds cat(h, vb), which ResidualBlock.run
    materialises with one plain nps_frame_pack (no GroupNorm, no pad4); the only other frame_pack is the final
    GroupNorm(8, 16) conv's (2 channels per group)."""
    _x3_only()
    s = _Spy(monkeypatch).run(M.find(hidden=16, n_cond=16, padding_mode="ones").id)
    assert [(c["C"], c["s2d_pad"]) for c in s.convs if c["s2d_pad"] is not None] == [
        ((16,), 1), ((16,), 1), ((32,), 1), ((16,), 1)] and s.s2d == []
    assert [(p["C"], p["gn"] is None, p["pad4"]) for p in s.packs[:-1]] == [((16, 16), True, False)]
    assert s.packs[-1]["gn"].groups == 8 and s.convs[-1]["packed"]
    assert not any(c["packed"] for c in s.convs[:-1])
    assert [c["phases"] for c in s.convs if c["out_os"] == 2] == [4, 4]  # one merged launch per Upsample
    assert set(s.classes) == {"x3f16"}
