"""SpectralConv1d / FNO_Layer / FNO in one dimension (reference proc_fno.py:158-222, :87-155, :22-83): the CPU side.

spectral1d_ref.py restates the contract in fp64 from its formulas; here it is pinned to every output of the
reference recorded in tests/golden/fno1d.pt (make_golden_1d.py).  The other tests: seeded construction reproduces
the fixture's state_dict bit for bit, the new ops and both module routes refuse CPU tensors, and the new C entry
points refuse shapes outside the documented envelope on the host, before any launch (the pointers below are dummy
integers).
"""
import pytest
import torch

from conftest import load_golden, rel_l2
from spectral1d_ref import CASES, SPECTRAL, build_module, call_module, case_ref

MAX_L, MAX_M = 65536, 128  # include/nps.h, the SpectralConv1d envelope


@pytest.fixture(scope="module")
def gold():
    return load_golden("fno1d")


# ------------------------------------------------------------------ the fp64 restatement
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(gold, name):
    g = gold[name]
    err = rel_l2(case_ref(name, g), g["y"])
    print(f"{name}: rel-L2 restatement vs reference {err:.3e}")
    assert err < 1e-6


def test_fixture_covers_nyquist_and_odd_lengths(gold):
    nyq, odd = gold["spectral1d_nyq"], gold["spectral1d_odd"]
    L = nyq["x"].shape[2]
    assert L % 2 == 0 and nyq["kwargs"]["modes"][0] == L // 2 + 1
    L = odd["x"].shape[2]
    assert L % 2 == 1 and odd["kwargs"]["modes"][0] == L // 2 + 1


# ------------------------------------------------------------------ construction
@pytest.mark.parametrize("name", CASES)
def test_seeded_construction_matches_the_fixture_bit_for_bit(gold, name):
    g = gold[name]
    sd = build_module(name, g["kwargs"]).state_dict()
    assert list(sd) == list(g["state_dict"])
    for k, v in sd.items():
        assert v.shape == g["state_dict"][k].shape and v.dtype == g["state_dict"][k].dtype, k
        assert torch.equal(v, g["state_dict"][k]), k
    assert set(g["grads"]) == set(sd)


def test_pointwise_conv1d_is_an_nn_conv1d():
    from torch import nn
    from models.common import get_conv_with_right_spatial_dim
    c = get_conv_with_right_spatial_dim(1, in_channels=3, out_channels=2, kernel_size=3, padding="same",
                                        padding_mode="circular")
    assert isinstance(c, nn.Conv1d) and not c.pointwise()
    y = c(torch.zeros(1, 3, 8))  # every geometry other than kernel 1 keeps nn.Conv1d's own forward
    assert y.shape == (1, 2, 8)
    with pytest.raises(NotImplementedError, match="pointwise"):
        c.run([], (1, 8))


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", ["spectral1d_a", "spectral1d_a_tm1", "fno_layer1d", "fno_layer1d_double", "fno1d_film",
                                  "fno1d_concat"])
def test_modules_refuse_cpu_tensors(gold, name):
    g = gold[name]
    m = build_module(name, g["kwargs"])
    with pytest.raises(RuntimeError, match="MI355X"):
        call_module(name, m, g["x"], g.get("p"), g.get("vb"))  # the autograd route
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        call_module(name, m, g["x"], g.get("p"), g.get("vb"))


def test_ops_refuse_cpu_tensors(gold):
    from nps_hip import ops
    from nps_hip import autograd as ad
    g = gold["spectral1d_a_tm1"]
    m = build_module("spectral1d_a_tm1", g["kwargs"])
    xl = g["x"].transpose(1, 2).contiguous()  # (B, L, C)
    c64 = torch.complex64
    calls = [
        lambda: ops.pack_spectral1d_weight(m.weights1),
        lambda: ops.spectral1d_dft([ops.Src(xl)], 4),
        lambda: ops.spectral1d_idft(torch.zeros(2, 4, 5, dtype=c64), 16),
        lambda: ops.film1d_scale((g["p"], m.weights_feat.weight, m.weights_feat.bias, 1), 2, 5, 4),
        lambda: ops.spectral_conv1d([ops.Src(xl)], torch.zeros(4, 6, 5, dtype=c64), 4, 5),
        lambda: ad.spectral_conv1d(m, xl),
        lambda: ad.spectral_conv1d_film(m, xl, g["p"]),
        lambda: m.run([ops.Src(xl)], p=g["p"]),
        lambda: m.run_ad(xl, g["p"]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
            pytest.fail(f"call {i} accepted CPU tensors")


def test_feature_transform_without_p_is_an_assertion_error(gold):
    g = gold["spectral1d_a_tm0"]
    m = build_module("spectral1d_a_tm0", g["kwargs"])
    with pytest.raises(AssertionError):
        m(g["x"])
    with torch.no_grad(), pytest.raises(AssertionError):
        m(g["x"])


def test_too_many_modes_is_an_assertion_error(gold):
    g = gold["spectral1d_a"]
    m = build_module("spectral1d_a", dict(g["kwargs"], modes=[10]))  # L = 16: at most 9
    with pytest.raises(AssertionError, match="modes"):
        m(g["x"])


def test_kernel_size_3_in_1d_is_refused_and_says_so():
    from models.enc_proc_dec_components.proc_fno import FNO_Layer, FNO
    layer = FNO_Layer(hidden_dim=4, num_spatial_dims=1, modes=3, kernel_size=3)
    x = torch.zeros(1, 4, 16)
    with pytest.raises(NotImplementedError, match="fno_kernel_size"):
        layer(x)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fno_kernel_size"):
        layer(x)
    fno = FNO(pde=None, num_spatial_dims=1, hidden_features=4, fno_modes=3, hidden_blocks=1, cond_mode=None,
              fno_kernel_size=3)
    with pytest.raises(NotImplementedError, match="fno_kernel_size"):
        fno(x)


def test_film_fno1d_without_variables_says_why():
    m = build_module("fno1d_film", dict(num_spatial_dims=1, n_cond=3, hidden_features=8, fno_modes=3, hidden_blocks=1,
                                        cond_mode="film"))
    with pytest.raises(NotImplementedError, match="does not route `variables`"):
        m(torch.zeros(1, 8, 16))


# ------------------------------------------------------------------ host checks of the C ABI
P, WF, BF, S, X, W1, Y, WS, DY, GS, Z = (0x1000 * i for i in range(1, 12))
B, K, CIN, COUT, L, M = 2, 3, 5, 4, 16, 4


def _err(rc):
    import nps_hip
    assert rc < 0
    return nps_hip.lib.nps_last_error().decode()


def _src(L=L, C=CIN, H=1):
    import nps_hip
    arr = (nps_hip.Src * 3)()
    arr[0].ptr, arr[0].C, arr[0].H, arr[0].W = X, C, H, L
    return arr


def test_stage_entry_points_check_the_envelope_before_any_launch():
    import nps_hip
    lib = nps_hip.lib
    dft = lambda L=L, m=M, nsrc=1, C=CIN, H=1: lib.nps_spectral1d_dft(_src(L, CIN, H), nsrc, B, L, C, m, Y, WS, 0, None)
    idft = lambda L=L, m=M, act=0: lib.nps_spectral1d_idft(Z, Y, B, L, m, COUT, 0, None, act, 0, None)
    for f in (dft, idft):
        assert "modes" in _err(f(m=L // 2 + 2))            # m > L // 2 + 1
        assert "modes" in _err(f(L=1024, m=MAX_M + 1))     # m above the cap
        assert "modes" in _err(f(m=0))
        assert "L must be" in _err(f(L=1, m=1))            # L < 2
        assert "L must be" in _err(f(L=MAX_L + 1))         # L above the documented cap
    assert "sources" in _err(dft(nsrc=4))
    assert "source 0" in _err(dft(H=2))
    assert "channels" in _err(dft(C=CIN + 1))
    assert "act" in _err(idft(act=2))
    assert "NULL" in _err(lib.nps_spectral1d_idft(None, Y, B, L, M, COUT, 0, None, 0, 0, None))
    assert lib.nps_spectral1d_dft_workspace(B, L, CIN, L // 2 + 2) == 0
    assert lib.nps_spectral1d_dft_workspace(B, MAX_L + 1, CIN, M) == 0
    assert lib.nps_spectral1d_dft_workspace(B, 4096, CIN, M) > 0


def test_film_entry_points_refuse_bad_transform_mode_and_k():
    import nps_hip
    lib = nps_hip.lib
    scale = lambda K=K, mode=0: lib.nps_spectral1d_film_scale(P, WF, BF, S, B, K, COUT, M, mode, None)
    pb = lambda K=K, mode=0: lib.nps_spectral1d_film_param_bwd(GS, P, WF, None, None, None, B, K, COUT, M, mode, None)
    for f in (scale, pb):
        assert "K" in _err(f(K=0))                          # K <= 0
        assert "K" in _err(f(K=-2))
        assert "K" in _err(f(K=65))
        assert "transform_mode" in _err(f(mode=2))
        assert "transform_mode" in _err(f(mode=-1))
    assert "NULL" in _err(lib.nps_spectral1d_film_scale(None, WF, BF, S, B, K, COUT, M, 0, None))
    assert "bad args" in _err(lib.nps_spectral1d_pack_weights(W1, WS, CIN, COUT, 0, None))
    assert "bad args" in _err(lib.nps_spectral1d_unpack_grad(WS, None, CIN, COUT, M, None))


def test_composites_check_their_arguments_before_any_launch():
    import nps_hip
    lib = nps_hip.lib

    def fwd(film, L=L, m=M, K=K, mode=0, p=P, act=0):
        if film:
            return lib.nps_spectral_conv1d_film_fwd(X, W1, p, WF, BF, Y, WS, B, CIN, COUT, L, m, K, mode, 0, act, None)
        return lib.nps_spectral_conv1d_fwd(X, W1, Y, WS, B, CIN, COUT, L, m, 0, act, None)

    def bwd(film, L=L, m=M, K=K, mode=0):
        if film:
            return lib.nps_spectral_conv1d_film_bwd(X, W1, P, WF, BF, DY, None, None, None, None, None, WS, B, CIN,
                                                    COUT, L, m, K, mode, None)
        return lib.nps_spectral_conv1d_bwd(X, W1, DY, None, None, WS, B, CIN, COUT, L, m, None)

    for film in (False, True):
        for f in (fwd, bwd):
            assert "modes" in _err(f(film, m=L // 2 + 2))
            assert "modes" in _err(f(film, L=1024, m=MAX_M + 1))
            assert "L must be" in _err(f(film, L=1, m=1))
            assert "L must be" in _err(f(film, L=MAX_L + 1))
        assert "act" in _err(fwd(film, act=3))
    for f in (fwd, bwd):
        assert "K" in _err(f(True, K=0))
        assert "K" in _err(f(True, K=-1))
        assert "transform_mode" in _err(f(True, mode=2))
    assert "NULL" in _err(fwd(True, p=None))
    assert "NULL" in _err(lib.nps_spectral_conv1d_fwd(X, W1, Y, None, B, CIN, COUT, L, M, 0, 0, None))
    assert lib.nps_spectral_conv1d_workspace(B, CIN, COUT, L, L // 2 + 2) == 0
    assert lib.nps_spectral_conv1d_workspace(B, CIN, COUT, 1, 1) == 0
    assert lib.nps_spectral_conv1d_film_workspace(B, CIN, COUT, MAX_L + 1, M) == 0
    assert (lib.nps_spectral_conv1d_film_workspace(B, CIN, COUT, L, M)
            > lib.nps_spectral_conv1d_workspace(B, CIN, COUT, L, M) > 0)


def test_python_mirrors_the_envelope():
    from nps_hip import ops
    assert (ops.SPECTRAL1D_MAX_L, ops.SPECTRAL1D_MAX_MODES) == (MAX_L, MAX_M)
    with pytest.raises(AssertionError, match="modes"):
        ops.check_modes1d(16, 10)
    with pytest.raises(NotImplementedError, match="modes"):
        ops.check_modes1d(1024, MAX_M + 1)
    with pytest.raises(NotImplementedError, match="L"):
        ops.check_modes1d(MAX_L + 2, 4)
    ops.check_modes1d(MAX_L, MAX_M)
    ops.check_modes1d(2, 2)
