"""The n-D EncProcDec restatement (tests/encprocdec_nd_ref.py) against the reference's recorded 1-D and 3-D models
(tests/golden/encprocdec_nd.pt, made by tests/golden/make_golden_encprocdec_nd.py), on the CPU.

  y: rel-L2 < 1e-6 in fp32 — both sides are fp32 aten on the CPU (the 1-D spectral conv of the restatement is an
     fp64 matrix product); BASELINE.md measures this noise floor at 1e-8 .. 3e-7.
  parameter gradients, fp64 restatement vs the reference's fp32 autograd: the _grads_ok rule of
     tests/test_gpu_unet3d_train.py (whole vector rel-L2 < 1e-5; per tensor < 1e-4, or an error below 1e-5 x the
     norm of the whole gradient).
"""
import ctypes

import pytest
import torch

from conftest import rel_l2
import encprocdec_nd_ref as R

from encprocdec_nd_ref import golden_case

CASES = ["epd1d_fno", "epd3d_fno"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_output(name):
    g = golden_case(name)
    with torch.no_grad():
        y = R.encprocdec_nd(g["state_dict"], g["kwargs"], g["pde"], g["x"], g["cond"], g["pos"],
                            g.get("spatial_cond"))
    err = rel_l2(y, g["y"])
    print(f"{name}: restatement vs reference y rel-L2 {err:.2e}")
    assert y.shape == g["x"].shape and err < 1e-6


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_gradients(name):
    g = golden_case(name)
    y, grads = R.reference_grads(g["state_dict"], g["kwargs"], g["pde"], g["x"], g["cond"], g["pos"],
                                 g.get("spatial_cond"), g["g"])
    assert rel_l2(y, g["y"]) < 1e-6
    assert set(grads) == set(g["grads"]) == set(g["state_dict"])
    R.grads_ok(g["grads"], grads)


def test_fixture_holds_what_the_cases_call_for():
    g1, g3 = golden_case("epd1d_fno"), golden_case("epd3d_fno")
    assert g1["x"].shape == (2, 2, 5, 72) and g1["pos"].shape == (2, 72) and g1["cond"].shape == (2, 2)
    assert g3["x"].shape == (2, 1, 25, 4, 6, 10) and g3["pos"].shape == (2, 4, 6, 10, 3)
    assert g3["cond"].shape == (2, 3) and g3["spatial_cond"].shape == (2, 1, 4, 6, 10)
    assert g1["state_dict"]["decoder.decoder.0.weight"].shape[2] == 3          # ka = 3, kb = 3: the generic kernel
    assert g1["state_dict"]["decoder.decoder.2.weight"].shape[2] == 3
    assert g3["state_dict"]["processor.0.fno_layers.0.conv.weights1"].shape == (20, 16, 3, 4, 3)
    for g in (g1, g3):
        assert g["pde"]["dt"] > 0 and g["g"].shape == g["y"].shape


def test_pack_nd_is_bound():
    """include/nps.h declares nps_pack_grid_input_nd and the library exports it (test_cabi checks every symbol); here
    its ctypes registration: 6 pointers, 7 ints (B, CT, N, P, K, S, Cp), the stream."""
    import nps_hip
    fn = nps_hip.lib.nps_pack_grid_input_nd
    assert "nps_pack_grid_input_nd" in nps_hip.EXPORTED
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
