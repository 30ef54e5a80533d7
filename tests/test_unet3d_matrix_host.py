"""The 3-D U-Net / U-FNO option matrix on the CPU: every row of tests/unet3d_matrix.py is a valid model for the
oracle, the fp64 use of the oracle is tied to the reference project's 3-D goldens, and the fp32 oracle sits far enough
below the GPU bar.  The state_dicts are the stand-in ones (oracle.functional.unet_structure's module list, seeded
weights): no project module and no shared library is loaded here.

Measured with these stand-in weights: rel-L2 of the fp32 oracle's output against the fp64 one 9.5e-8 ... 8.6e-7 over
the 26 rows (the smallest on the norm=False rows, the largest on the hidden-16 norm rows with a 3x3x3 final conv and the
hidden-32 two-block rows), so the bound stays 1e-6 and the GPU bar of 1e-5 keeps more than 10x over an exact fp32
evaluation.  Two U-FNO rows were moved to another grid to fit (unet3d_matrix._ufno_rows).  The whole file runs in
about 11 s (the slowest row, C5's structure, takes 2 s for its fp64 forward and backward).
"""
import functools

import pytest
import torch

from conftest import load_golden, rel_l2
from oracle import functional as Fo
import unet3d_matrix as M

FP32_VS_FP64 = 1e-6
GOLDEN_TOL = 1e-5   # tests/test_oracle_golden.py::TOL, the fp32 oracle's bar against the same goldens

# Parameters whose gradient is analytically zero.
# * hidden 8: the final GroupNorm(8, 8) is per channel, and a per-channel constant added to its input cancels in it.
#   The last UpBlock's shortcut bias is such a constant; its conv2 bias is not (every 3-D conv here is a valid conv
#   whose output crop_Nd zero-pads back: the bias reaches the interior only), as on the 2-D matrix's circular row.
# * the C5-structure row, modes (8, 12, 12) on (11, 12, 22): m2 = 12 = H, so the corners [:m1, -m2:] and
#   [-m1:, -m2:] that SpectralConv3d writes with weights3 / weights4 (proc_fno.py:334-376, later assignments win)
#   cover the whole of the corners written with weights1 / weights2 before them: weights1 and weights2 do not reach
#   the output at all.
_C5_DEAD = {f"fno_layers.0.conv.weights{n}" for n in (1, 2)}
ZERO_GRADS = {
    "unet-h8-m12-b2-circ-gn-k1-c2-11x12x13-B3": {"up.6.res.shortcut.bias"},
    M.C5_ROW.id: _C5_DEAD,
}


@functools.lru_cache(maxsize=None)
def _run(rid):
    row = M.BY_ID[rid]
    sd = M.standin_state_dict(row)
    h, vb, gy = M.inputs(row)
    return sd, (h, vb, gy), M.reference(row, sd, h, vb, gy)


def test_the_table_is_what_the_matrix_promises():
    def cases(kind="unet", **kw):
        return [r.case for r in M.ROWS if r.kind == kind and all(getattr(r.case, k) == v for k, v in kw.items())]

    core = cases(hidden=16, ch_mults=(1, 2), n_blocks=1, B=2)
    core = [c for c in core if c.n_cond in (0, 4)]
    at0 = {(c.norm, c.use1x1, c.n_cond) for c in core if c.dhw == (11, 12, 13)}
    assert len(at0) == 8
    at1 = [c for c in core if c.dhw == (14, 12, 11)]
    assert len(at1) == 2 and len(core) == 10
    assert {c.norm for c in at1} == {c.use1x1 for c in at1} == {True, False} and {c.n_cond for c in at1} == {0, 4}
    # channel alignment
    assert cases(hidden=8, ch_mults=(1, 2), n_blocks=2, n_cond=2, B=3, norm=True) != []
    assert cases(hidden=24, ch_mults=(1, 2), n_cond=4, norm=True) != []
    assert cases(hidden=6, ch_mults=(2, 1), norm=False, use1x1=False, n_cond=1, dhw=(11, 11, 12)) != []
    # identity shortcuts: on a concatenation (U-Net and U-FNO), on a single source without and with conditioning
    assert len(cases(hidden=16, n_cond=16, ch_mults=(1, 2))) == 1
    assert len(cases(kind="ufno", hidden=16, n_cond=16, ch_mults=(1, 2))) == 1
    assert sorted(c.n_cond for c in cases(hidden=32, ch_mults=(2, 1), n_blocks=2)) == [0, 4]
    # wide
    assert len(cases(hidden=48, ch_mults=(2, 2), n_cond=4, B=1, dhw=(11, 11, 12))) == 1
    assert len(cases(hidden=64, ch_mults=(2, 2), n_cond=4, B=1)) == 1
    from bench import C5_UFNO_CFG
    (c5,) = cases(kind="c5")
    assert (c5.hidden, list(c5.ch_mults), c5.n_blocks, c5.norm, c5.use1x1, c5.n_cond, c5.B) == tuple(
        C5_UFNO_CFG[k] for k in ("hidden_features", "ch_mults", "n_blocks", "norm", "use1x1", "n_cond")) + (1,)
    assert M.ufno_modes(M.C5_ROW) == tuple(C5_UFNO_CFG["fno_modes"])
    # depth, borders and tiny grids
    assert len(cases(ch_mults=(1, 1, 2), hidden=16, n_cond=4, B=1, dhw=(23, 24, 25))) == 1
    assert M.ZERO_BORDER_ROW.case == M.Case(16, (1,), 1, True, False, 4, (6, 7, 9), 2)
    assert M.UFNO_BORDER_ROW.case == M.ZERO_BORDER_ROW.case and M.UFNO_BORDER_ROW.kind == "ufno"
    assert len(cases(ch_mults=(1,), dhw=(5, 5, 6), B=1)) == 1
    # U-FNO
    ufno = cases(kind="ufno")
    assert len(ufno) == 4 and sorted(c.n_cond for c in ufno) == [0, 4, 4, 16]
    assert sorted(c.n_cond for c in cases(kind="ufno", hidden=16, ch_mults=(1, 1))) == [0, 4]
    assert len(M.ROWS) == 26 and len(ZERO_GRADS.keys() - M.BY_ID.keys()) == 0
    assert [r.kind for r in M.BF16_ROWS] == ["unet", "c5", "ufno", "unet"] and M.BF16_REFUSED.keys() <= M.BY_ID.keys()
    assert M.BF16_ROWS[0].case == M.Case(16, (1, 2), 1, True, True, 4, (11, 12, 13), 2)


def test_geometry_rules():
    """The lowest level of every row keeps 5 voxels per axis (the two valid 3x3x3 convs of a block shrink 5 to 1), and
    every U-FNO row's modes lie inside the HIP spectral envelope (ops.check_modes3d: m1 <= D, m2 <= H,
    m3 <= W // 2 + 1).  hidden % 8 != 0 rows have norm=False (the final norm is GroupNorm(8, hidden))."""
    assert M.level_extents((11, 12, 13), 2)[-1] == (5, 5, 6) and M.level_extents((23, 24, 25), 3)[-1] == (5, 5, 5)
    assert min(M.level_extents((10, 12, 13), 2)[-1]) < 5 and min(M.level_extents((22, 24, 25), 3)[-1]) < 5
    for r in M.ROWS:
        c = r.case
        assert min(M.level_extents(c.dhw, len(c.ch_mults))[-1]) >= 5, r.id
        assert c.hidden % 8 == 0 or not c.norm, r.id
        if M.is_ufno(r):
            (m1, m2, m3), (D, H, W) = M.ufno_modes(r), c.dhw
            assert m1 <= D and m2 <= H and m3 <= W // 2 + 1, r.id
    # the C5 row's grid is the smallest one: one voxel less on any axis leaves the envelope or the two-level minimum
    (m1, m2, m3), (D, H, W) = M.ufno_modes(M.C5_ROW), M.C5_ROW.case.dhw
    assert D - 1 < 11 and H - 1 < m2 and (W - 1) // 2 + 1 < m3


def test_an_axis_below_the_minimum_fails_in_the_oracle_itself():
    row = M._row("unet", 16, (1, 2), 1, True, True, 4, (10, 12, 13), 1)
    sd = M.standin_state_dict(M.find(hidden=16, ch_mults=(1, 2), norm=True, use1x1=True, n_cond=4, dhw=(11, 12, 13)))
    h, vb, _ = M.seeded_inputs(row.case, row.case.dhw, 1)
    with pytest.raises(RuntimeError, match="Kernel size can't be greater than actual input size"):
        M.reference(row, sd, h, vb)


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_runs_in_the_fp64_oracle_and_every_parameter_gets_a_gradient(rid):
    row = M.BY_ID[rid]
    sd, (h, vb, gy), ref = _run(rid)
    assert ref.y.dtype == torch.float64 and ref.y.shape == h.shape and torch.isfinite(ref.y).all()
    assert ref.dh.shape == h.shape and torch.isfinite(ref.dh).all() and ref.dh.abs().max() > 0
    assert (ref.dvb is None) == (row.case.n_cond == 0) == (vb is None)
    if ref.dvb is not None:
        assert ref.dvb.shape == vb.shape and torch.isfinite(ref.dvb).all() and ref.dvb.abs().max() > 0
    assert set(ref.grads) == set(sd)
    for k, g in ref.grads.items():
        assert g is not None and g.shape == sd[k].shape and torch.isfinite(torch.view_as_real(g) if g.is_complex()
                                                                           else g).all(), k
        assert g.dtype == (torch.complex128 if sd[k].is_complex() else torch.float64)
    gmax = max(g.abs().max().item() for g in ref.grads.values())
    zero = {k for k, g in ref.grads.items() if g.abs().max().item() <= 1e-10 * gmax}
    assert zero == ZERO_GRADS.get(rid, set())


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_standin_state_dict_has_the_3d_shapes(rid):
    sd = M.standin_state_dict(M.BY_ID[rid])
    for k, v in sd.items():
        if k.endswith("weight") and ".norm" not in k and not k.startswith("norm"):
            assert v.dim() == 5 and len(set(v.shape[2:])) == 1, k
            if ".up." in "." + k and k.endswith("conv.weight"):   # Upsample: (Cin, Cout, 4, 4, 4)
                assert v.shape[2] == 4 and v.shape[0] == v.shape[1], k
            else:
                assert v.shape[2] in (1, 3), k
        elif ".conv.weights" in k:
            assert v.dtype == torch.complex64 and tuple(v.shape[2:]) == M.ufno_modes(M.BY_ID[rid]), k


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_fp32_oracle_is_within_1e6_of_the_fp64_one(rid):
    row = M.BY_ID[rid]
    sd, (h, vb, _), ref = _run(rid)
    y32 = M.reference(row, sd, h, vb, None, torch.float32).y
    assert y32.dtype == torch.float32
    e = rel_l2(y32, ref.y)
    print(f"{rid}: fp32 oracle vs fp64 oracle rel-L2 {e:.2e}")
    assert e < FP32_VS_FP64


def _f64(t):
    return t.to(torch.complex128 if t.is_complex() else torch.float64)


@pytest.mark.parametrize("name,fn", [("unet3d_single", Fo.unet_modern3d), ("ufno3d_single", Fo.ufno3d)])
def test_fp64_oracle_reproduces_the_reference_goldens(name, fn):
    g = load_golden(name)
    kw = dict(g["kwargs"], n_cond=2) if name == "unet3d_single" else g["kwargs"]  # (as tests/test_oracle_golden.py)
    with torch.no_grad():
        y = fn({k: _f64(v) for k, v in g["state_dict"].items()}, "", kw, _f64(g["h"]), _f64(g["vb"]))
    assert y.dtype == torch.float64 and y.shape == g["y"].shape
    assert rel_l2(y, g["y"]) < GOLDEN_TOL


def test_fp64_oracle_reproduces_the_downsample3d_golden():
    g = load_golden("downsample3d")
    sd = {k: _f64(v) for k, v in g["state_dict"].items()}
    yh = Fo.conv3d_ref(_f64(g["h"]), sd, "conv", stride=2, padding_mode="circular")
    yv = Fo.conv3d_ref(_f64(g["vb"]), sd, "conv_variables_broadcast", stride=2, padding_mode="circular")
    assert yh.dtype == torch.float64 and yh.shape == g["yh"].shape and yv.shape == g["yv"].shape
    assert rel_l2(yh, g["yh"]) < GOLDEN_TOL and rel_l2(yv, g["yv"]) < GOLDEN_TOL


def _shell(shape):
    s = torch.ones(shape, dtype=torch.bool)
    s[1:-1, 1:-1, 1:-1] = False
    return s


def test_zero_border_row_has_an_exactly_zero_outer_shell():
    """ch_mults (1,), 3x3x3 final conv: the final conv's valid output is 2 smaller per axis than the input and crop_Nd
    pads it with zeros (offsets (1, 1, 1) in UNetModern.run3d).  The layer just inside the shell is not zero."""
    _, _, ref = _run(M.ZERO_BORDER_ROW.id)
    y = ref.y
    shell = _shell(y.shape[-3:])
    assert (y[..., shell] == 0).all()
    inner = ~shell
    inner[1:-1, 1:-1, 1:-1] &= _shell(tuple(n - 2 for n in y.shape[-3:]))
    assert inner.sum() == 4 * 5 * 7 - 2 * 3 * 5 and (y[..., inner] != 0).all()


def test_ufno_border_row_needs_the_activated_addend_on_its_shell():
    """The same geometry under a U-FNO: the block output's shell is gelu(h_fno + 0), which is not zero."""
    _, _, ref = _run(M.UFNO_BORDER_ROW.id)
    y = ref.y
    for ax in (-3, -2, -1):
        assert (y.select(ax, 0) != 0).any() and (y.select(ax, y.shape[ax] - 1) != 0).any()
