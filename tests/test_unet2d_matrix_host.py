"""The 2-D U-Net / U-FNO option matrix on the CPU: every row of tests/unet2d_matrix.py is a valid model for the
oracle, the fp64 use of the oracle is tied to the reference project's goldens, and the fp32 oracle sits far enough
below the GPU bar.  The state_dicts are the stand-in ones (oracle.functional.unet_structure's module list, seeded
weights): no project module and no shared library is loaded here.

Measured with these stand-in weights (and with the modules' own initialisation, which gives the same range):
rel-L2 of the fp32 oracle's output against the fp64 one 4.7e-8 ... 7.3e-7 over the 44 rows (the smallest on the
3 x 3 grid, the largest on the U-FNO rows and the 64 x 64 four-level row), so the bound stays 1e-6 and the GPU bar
of 1e-5 keeps more than 10x over an exact fp32 evaluation.  The whole file runs in about 5 s.
"""
import functools

import pytest
import torch

from conftest import load_golden, rel_l2
from oracle import functional as Fo
import unet2d_matrix as M

FP32_VS_FP64 = 1e-6
GOLDEN_TOL = 1e-5   # tests/test_oracle_golden.py::TOL, the fp32 oracle's bar against the same goldens

# Parameters whose gradient is analytically zero (tests/test_gpu_backward.py::_grads_ok's docstring): at hidden 8
# the final GroupNorm(8, 8) is per channel, and a per-channel constant added to its input cancels in it.  The last
# UpBlock's shortcut bias is such a constant; so is its conv2 bias under 'ones' (conv2's output covers the whole
# map), but not under 'circular' (its valid-conv output is zero-padded back by crop_Nd: the bias reaches the interior
# only and is no longer constant over the map).
ZERO_GRADS = {
    "unet-h8-m12-b2-ones-gn-k1-c2-21x18-B3": {"up.6.res.conv2.bias", "up.6.res.shortcut.bias"},
    "unet-h8-m12-b2-circ-gn-k1-c2-21x18-B3": {"up.6.res.shortcut.bias"},
}


@functools.lru_cache(maxsize=None)
def _run(rid):
    row = M.BY_ID[rid]
    sd = M.standin_state_dict(row)
    h, vb, gy = M.inputs(row)
    return sd, (h, vb, gy), M.reference(row, sd, h, vb, gy)


def test_the_table_is_what_the_matrix_promises():
    core = [r.case for r in M.ROWS if r.kind == "unet" and r.case.hidden == 16 and r.case.ch_mults == (1, 2)]
    at21 = {(c.padding_mode, c.norm, c.use1x1, c.n_cond) for c in core if c.hw == (21, 18)}
    assert len(at21) == 16 and all(c.n_blocks == 1 and c.B == 2 for c in core)
    at24 = [c for c in core if c.hw == (24, 20)]
    assert len(at24) == 4 and {c.padding_mode for c in at24} == {"ones", "circular"}
    assert {c.n_cond for c in at24} == {0, 4}
    assert len(ZERO_GRADS.keys() - M.BY_ID.keys()) == 0
    ufno = [r.case for r in M.ROWS if r.kind == "ufno"]
    assert len(ufno) == 4 and sorted(c.n_cond for c in ufno) == [0, 4, 4, 4]
    for r in M.ROWS:  # the HIP spectral path's envelope (SpectralConv2d: modes1 <= H, modes2 <= W // 2 + 1)
        if r.kind == "ufno":
            assert M.UFNO_MODES <= r.case.hw[0] and M.UFNO_MODES <= r.case.hw[1] // 2 + 1


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_runs_in_the_fp64_oracle_and_every_parameter_gets_a_gradient(rid):
    row = M.BY_ID[rid]
    sd, (h, vb, gy), ref = _run(rid)
    assert ref.y.dtype == torch.float64 and ref.y.shape == h.shape and torch.isfinite(ref.y).all()
    assert ref.dh.shape == h.shape and ref.dh.abs().max() > 0
    assert (ref.dvb is None) == (row.case.n_cond == 0)
    if ref.dvb is not None:
        assert ref.dvb.shape == vb.shape and ref.dvb.abs().max() > 0
    assert set(ref.grads) == set(sd)
    for k, g in ref.grads.items():
        assert g is not None and g.shape == sd[k].shape and torch.isfinite(torch.view_as_real(g) if g.is_complex()
                                                                           else g).all(), k
    gmax = max(g.abs().max().item() for g in ref.grads.values())
    zero = {k for k, g in ref.grads.items() if g.abs().max().item() <= 1e-10 * gmax}
    assert zero == ZERO_GRADS.get(rid, set())


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_fp32_oracle_is_within_1e6_of_the_fp64_one(rid):
    row = M.BY_ID[rid]
    sd, (h, vb, _), ref = _run(rid)
    y32 = M.reference(row, sd, h, vb, None, torch.float32).y
    assert y32.dtype == torch.float32
    e = rel_l2(y32, ref.y)
    print(f"{rid}: fp32 oracle vs fp64 oracle rel-L2 {e:.2e}")
    assert e < FP32_VS_FP64


@pytest.mark.parametrize("name,fn", [("unet_ufno_style", Fo.unet_modern), ("unet_cfg", Fo.unet_modern),
                                     ("unet_ones", Fo.unet_modern), ("ufno", Fo.ufno)])
def test_fp64_oracle_reproduces_the_reference_goldens(name, fn):
    g = load_golden(name)
    f64 = lambda t: t.to(torch.complex128 if t.is_complex() else torch.float64)  # noqa: E731
    with torch.no_grad():
        y = fn({k: f64(v) for k, v in g["state_dict"].items()}, "", g["kwargs"], f64(g["h"]), f64(g["vb"]))
    assert y.dtype == torch.float64 and y.shape == g["y"].shape
    assert rel_l2(y, g["y"]) < GOLDEN_TOL


def test_zero_border_row_has_an_exactly_zero_outer_ring():
    """ch_mults [1], circular, 3x3 final conv: the final conv's valid output is 2 smaller than the input and crop_Nd
    pads it with zeros: oy = ox = 1 > 0 in UNetModern.run.  The interior next to the ring is not zero."""
    _, _, ref = _run(M.ZERO_BORDER_ROW.id)
    y = ref.y
    ring = torch.ones(y.shape[-2:], dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert (y[..., ring] == 0).all()
    inner = torch.zeros_like(ring)
    inner[1:-1, 1:-1] = True
    inner[2:-2, 2:-2] = False
    assert (y[..., inner] != 0).all()


def test_ufno_border_row_needs_the_activated_addend_on_its_ring():
    """The same geometry under a U-FNO: the block output's ring is gelu(h_fno + 0), which is not zero."""
    _, _, ref = _run(M.UFNO_BORDER_ROW.id)
    y = ref.y
    assert (y[..., 0, :] != 0).any() and (y[..., :, 0] != 0).any()
    assert (y[..., -1, :] != 0).any() and (y[..., :, -1] != 0).any()
