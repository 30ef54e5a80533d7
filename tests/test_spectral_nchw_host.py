"""CPU checks of the channels-first spectral C ABI: the new entry points are exported and bound, and their host-side
refusals (batch stride, mode bound, NULL pointer, row length past the LDS table) return an error with a message
before any launch or pointer dereference — the pointers below are dummy integers."""
import pytest

NCHW_NAMES = (
    "nps_spectral_dft_w_nchw", "nps_spectral_idft_w_nchw", "nps_spectral_idft_w_bwd_nchw",
    "nps_spectral_dft_w_bwd_nchw", "nps_spectral_conv2d_fwd_nchw", "nps_spectral_conv2d_bwd_nchw",
    "nps_spectral_conv3d_fwd_nchw", "nps_spectral_conv3d_bwd_nchw",
)
X, W1, W2, Y, WS, DY, DX = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
B, CIN, COUT, H, W, M1, M2 = 2, 5, 3, 6, 8, 2, 3


def test_nchw_entry_points_are_exported_and_declared():
    import os
    import re
    import nps_hip
    from conftest import ROOT
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nps.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nps_\w+)\s*\(", src))
    for n in NCHW_NAMES:
        assert n in nps_hip.EXPORTED and n in declared and hasattr(nps_hip.lib, n), n
    assert set(declared) == set(nps_hip.EXPORTED)


def _err(rc):
    import nps_hip
    assert rc < 0
    return nps_hip.lib.nps_last_error().decode()


def _fwd2(x_bs=0, y_bs=0, m2=M2, ws=WS):
    import nps_hip
    return nps_hip.lib.nps_spectral_conv2d_fwd_nchw(X, x_bs, W1, W2, Y, y_bs, ws, B, CIN, COUT, H, W, M1, m2, 0, 0,
                                                    None)


def _bwd2(x_bs=0, dy_bs=0, dx_bs=0, m2=M2, ws=WS):
    import nps_hip
    return nps_hip.lib.nps_spectral_conv2d_bwd_nchw(X, x_bs, W1, W2, DY, dy_bs, DX, dx_bs, None, None, ws, B, CIN, COUT,
                                                    H, W, M1, m2, None)


def test_conv2d_nchw_refuses_a_short_or_negative_batch_stride():
    assert "batch stride" in _err(_fwd2(x_bs=CIN * H * W - 1))
    assert "batch stride" in _err(_fwd2(y_bs=COUT * H * W - 1))
    assert "batch stride" in _err(_fwd2(x_bs=-CIN * H * W))
    assert "batch stride" in _err(_bwd2(x_bs=CIN * H * W - 1))
    assert "batch stride" in _err(_bwd2(dy_bs=-1))
    assert "batch stride" in _err(_bwd2(dx_bs=CIN * H * W - 1))


def test_conv2d_nchw_refuses_bad_modes_and_null_workspace():
    assert "modes" in _err(_fwd2(m2=W // 2 + 2))
    assert "bad shape" in _err(_bwd2(m2=W // 2 + 2))
    assert "NULL" in _err(_fwd2(ws=None))
    assert "NULL" in _err(_bwd2(ws=None))


def test_conv3d_nchw_host_checks():
    import nps_hip
    lib = nps_hip.lib
    D = 4
    w = [W1, W2, 0x8000, 0x9000]

    def fwd(x_bs=0, y_bs=0, m3=M2, ws=WS):
        return lib.nps_spectral_conv3d_fwd_nchw(X, x_bs, *w, Y, y_bs, ws, B, CIN, COUT, D, H, W, 2, M1, m3, 0, 0, None)

    def bwd(x_bs=0, dy_bs=0, dx_bs=0, ws=WS):
        return lib.nps_spectral_conv3d_bwd_nchw(X, x_bs, *w, DY, dy_bs, DX, dx_bs, None, None, None, None, ws, B, CIN,
                                                COUT, D, H, W, 2, M1, M2, None)
    assert "batch stride" in _err(fwd(x_bs=CIN * D * H * W - 1))
    assert "batch stride" in _err(fwd(y_bs=-1))
    assert "modes" in _err(fwd(m3=W // 2 + 2))
    assert "NULL" in _err(fwd(ws=None))
    assert "batch stride" in _err(bwd(dx_bs=CIN * D * H * W - 1))
    assert "batch stride" in _err(bwd(dy_bs=-5))
    assert "NULL" in _err(bwd(ws=None))


def test_w_pass_stages_check_their_arguments_on_the_host():
    import nps_hip
    lib = nps_hip.lib
    X1 = 0xa000
    assert "batch stride" in _err(lib.nps_spectral_dft_w_nchw(X, CIN * H * W - 1, B, H, W, CIN, M2, X1, None))
    assert "batch stride" in _err(lib.nps_spectral_idft_w_nchw(X1, Y, -1, B, H, W, M2, COUT, 0, 0, None))
    assert "batch stride" in _err(lib.nps_spectral_idft_w_bwd_nchw(DY, COUT * H * W - 1, X1, B, H, W, M2, COUT, None))
    assert "batch stride" in _err(lib.nps_spectral_dft_w_bwd_nchw(X1, DX, -7, B, H, W, M2, CIN, None))
    assert "m2" in _err(lib.nps_spectral_dft_w_nchw(X, 0, B, H, W, CIN, W // 2 + 2, X1, None))
    assert "NULL" in _err(lib.nps_spectral_dft_w_nchw(None, 0, B, H, W, CIN, M2, X1, None))
    assert "NULL" in _err(lib.nps_spectral_idft_w_nchw(X1, None, 0, B, H, W, M2, COUT, 0, 0, None))
    assert "act" in _err(lib.nps_spectral_idft_w_nchw(X1, Y, 0, B, H, W, M2, COUT, 0, 2, None))
    # a row whose twiddle table does not fit the LDS limit is refused, never launched
    assert "too large" in _err(lib.nps_spectral_dft_w_nchw(X, 0, 1, 2, 1000, CIN, M2, X1, None))


def test_ops_nchw_refuse_cpu_tensors():
    """No CPU fallback: a CPU tensor is an error, as for the other ops."""
    import torch
    from nps_hip import ops
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.spectral_conv2d_nchw(torch.zeros(1, 2, 4, 4), torch.zeros(2, 1, 2, 2, dtype=torch.complex64), 1, 1, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.spectral_conv3d_nchw(torch.zeros(1, 2, 4, 4, 4), None, 1, 1, 1, 2)
