"""FiLM conditioning of SpectralConv2d / FNO_Layer / FNO (reference proc_fno.py:271-284): the CPU side.

`film_scale_ref` / `film_spectral_ref` restate the contract in fp64 with torch.fft — the factor S from its closed
form (row by row: low corner, high corner, both where 2*m1 > H), not from the reference's slice assignments — and
are pinned here to every output of the reference recorded in tests/golden/film.pt (make_golden_film.py).  The GPU
tests (test_gpu_film.py) use them, with autograd, as the reference at shapes the fixture does not cover.

The other tests: seeded construction reproduces the fixture's state_dict bit for bit, the new ops refuse CPU
tensors, and the new C entry points refuse a bad transform_mode / K on the host, before any launch (the pointers
below are dummy integers).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2

SPECTRAL = [f"{n}_tm{tm}" for n in ("spectral2d_a", "spectral2d_overlap", "spectral2d_nyq") for tm in (0, 1)]


# ------------------------------------------------------------------ the fp64 restatement
def film_scale_ref(p, Wf, bf, Cout, H, m1, m2, mode):
    """S (B, Cout, H, m2) fp64 over every frequency row k1 (1 on rows outside both corners, where Y is zero)."""
    p, Wf, bf = p.double(), Wf.double(), bf.double()
    Fw = (p @ Wf.t() + bf).view(p.shape[0], Cout, 2 * m1, m2)  # F[b][n(o, j, k2)]
    rows = []
    for k1 in range(H):
        low, high = k1 < m1, k1 >= H - m1
        f_lo = Fw[:, :, k1] if low else None
        f_hi = Fw[:, :, k1 - (H - 2 * m1)] if high else None
        if mode == 0:
            s = torch.ones_like(Fw[:, :, 0])
            if low:
                s = s + f_lo
            if high:
                s = s + f_hi
        else:
            s = f_hi if high else (f_lo if low else torch.ones_like(Fw[:, :, 0]))
        rows.append(s)
    return torch.stack(rows, dim=2)


def mixed_modes_ref(x, w1, w2):
    """The unscaled retained spectrum (B, Cout, H, m2) complex128: the two corner products, the second winning."""
    m1, m2 = w1.shape[2], w1.shape[3]
    xf = torch.fft.rfft2(x.double())
    B, H = x.shape[0], x.shape[2]
    Y = torch.zeros(B, w1.shape[1], H, m2, dtype=torch.complex128)
    Y[:, :, :m1] = torch.einsum("bixy,ioxy->boxy", xf[:, :, :m1, :m2], w1.to(torch.complex128))
    Y[:, :, H - m1:] = torch.einsum("bixy,ioxy->boxy", xf[:, :, H - m1:, :m2], w2.to(torch.complex128))
    return Y


def film_spectral_ref(x, w1, w2, p, Wf, bf, mode):
    """SpectralConv2d with FiLM, (B, Cin, H, W) -> (B, Cout, H, W), fp64."""
    B, _, H, W = x.shape
    Cout, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
    Y = mixed_modes_ref(x, w1, w2) * film_scale_ref(p, Wf, bf, Cout, H, m1, m2, mode)
    out_ft = torch.zeros(B, Cout, H, W // 2 + 1, dtype=torch.complex128)
    out_ft[..., :m2] = Y
    return torch.fft.irfft2(out_ft, s=(H, W))


def _conv_film(sd, prefix, x, p, mode):
    return film_spectral_ref(x, sd[prefix + "weights1"], sd[prefix + "weights2"], p, sd[prefix + "weights_feat.weight"],
                             sd[prefix + "weights_feat.bias"], mode)


def fno_layer_ref(sd, prefix, x, p):
    """FNO_Layer (conv_mode single, kernel 1, GELU) with its default transform_mode 0, fp64."""
    w = F.conv2d(x.double(), sd[prefix + "w.weight"].double(), sd[prefix + "w.bias"].double())
    return F.gelu(_conv_film(sd, prefix + "conv.", x, p, 0) + w)


def case_ref(name, g):
    sd, x, p = g["state_dict"], g["x"], g["p"]
    if name == "fno_layer":
        return fno_layer_ref(sd, "", x, p)
    if name == "fno":
        h = x
        for i in range(g["kwargs"]["hidden_blocks"]):
            h = fno_layer_ref(sd, f"fno_layers.{i}.", h, p)
        return h
    return _conv_film(sd, "", x, p, g["kwargs"]["transform_mode"])


@pytest.fixture(scope="module")
def film():
    return load_golden("film")


@pytest.mark.parametrize("name", SPECTRAL + ["fno_layer", "fno"])
def test_restatement_reproduces_the_reference(film, name):
    g = film[name]
    err = rel_l2(case_ref(name, g), g["y"])
    print(f"{name}: rel-L2 restatement vs reference {err:.3e}")
    assert err < 1e-6


def test_overlap_case_has_rows_in_both_corners(film):
    """The overlap fixture is the one where the two transform_modes differ in kind (both terms vs second wins)."""
    kw = film["spectral2d_overlap_tm0"]["kwargs"]
    H = film["spectral2d_overlap_tm0"]["x"].shape[2]
    assert 2 * kw["modes"][0] > H


# ------------------------------------------------------------------ construction
def build_module(name, kwargs):
    """The product module of a fixture case, constructed as make_golden_film.py constructs the reference's."""
    from torch import nn  # noqa: F401
    from models.enc_proc_dec_components.proc_fno import SpectralConv2d, FNO_Layer, FNO
    torch.manual_seed(42)
    if name == "fno_layer":
        return FNO_Layer(**dict(kwargs, modes=tuple(kwargs["modes"])))
    if name == "fno":
        return FNO(pde=None, **kwargs)
    return SpectralConv2d(**dict(kwargs, modes=tuple(kwargs["modes"])))


@pytest.mark.parametrize("name", SPECTRAL + ["fno_layer", "fno"])
def test_seeded_construction_matches_the_fixture_bit_for_bit(film, name):
    g = film[name]
    sd = build_module(name, g["kwargs"]).state_dict()
    assert list(sd) == list(g["state_dict"])
    assert any(k.endswith("weights_feat.weight") for k in sd)
    for k, v in sd.items():
        assert v.shape == g["state_dict"][k].shape and v.dtype == g["state_dict"][k].dtype, k
        assert torch.equal(v, g["state_dict"][k]), k
    assert set(g["grads"]) == set(sd)


# ------------------------------------------------------------------ refusals
def test_film_ops_refuse_cpu_tensors(film):
    from nps_hip import ops
    g = film["spectral2d_a_tm1"]
    m = build_module("spectral2d_a_tm1", g["kwargs"])
    with pytest.raises(RuntimeError, match="MI355X"):
        m(g["x"], g["p"])  # the autograd route
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        m(g["x"], g["p"])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.film_scale((g["p"], m.weights_feat.weight, m.weights_feat.bias, 1), 2, 5, 16, 4, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.spectral_mix(torch.zeros(1), torch.zeros(1), torch.zeros(1), 1, 1, 1, 1, 1, S=torch.zeros(1))


def test_feature_transform_without_p_is_an_assertion_error(film):
    g = film["spectral2d_a_tm0"]
    m = build_module("spectral2d_a_tm0", g["kwargs"])
    with pytest.raises(AssertionError):
        m(g["x"])


def test_film_fno_without_variables_says_why():
    m = build_module("fno", dict(num_spatial_dims=2, n_cond=3, hidden_features=8, fno_modes=3, hidden_blocks=1,
                                 cond_mode="film"))
    with pytest.raises(NotImplementedError, match="does not route `variables`"):
        m(torch.zeros(1, 8, 16, 12))


def test_film_fno_without_conditioning_scalars_is_a_plain_fno():
    """cond_mode="film" with n_cond == 0 builds layers without feature_transform and needs no `variables`."""
    m = build_module("fno", dict(num_spatial_dims=2, n_cond=0, hidden_features=8, fno_modes=3, hidden_blocks=1,
                                 cond_mode="film"))
    assert not m.fno_layers[0].conv.feature_transform
    assert m._film_p(None) is None


def test_3d_film_message_names_the_reference_defect():
    from models.enc_proc_dec_components.proc_fno import SpectralConv3d
    m = SpectralConv3d(2, 2, (2, 2, 2), feature_transform=True, feature_transform_dim=3)
    with pytest.raises(NotImplementedError, match="cannot run"):
        m(torch.zeros(1, 2, 4, 4, 4))
    fno = build_module("fno", dict(num_spatial_dims=3, n_cond=3, hidden_features=4, fno_modes=2, hidden_blocks=1,
                                   cond_mode="film"))
    with pytest.raises(NotImplementedError, match="cannot run"):
        fno(torch.zeros(1, 4, 4, 4, 4), variables=torch.zeros(1, 3))


P, WF, BF, S, X, W1, W2, Y, WS, DY, GS = (0x1000 * i for i in range(1, 12))
B, K, CIN, COUT, H, W, M1, M2 = 2, 3, 5, 4, 6, 8, 2, 3


def _err(rc):
    import nps_hip
    assert rc < 0
    return nps_hip.lib.nps_last_error().decode()


def test_film_abi_refuses_bad_transform_mode_and_k():
    import nps_hip
    lib = nps_hip.lib
    scale = lambda K=K, mode=0, m1=M1, H=H: lib.nps_spectral_film_scale(P, WF, BF, S, B, K, COUT, H, m1, M2, mode, None)
    assert "K" in _err(scale(K=0))
    assert "K" in _err(scale(K=65))
    assert "transform_mode" in _err(scale(mode=2))
    assert "transform_mode" in _err(scale(mode=-1))
    assert "modes" in _err(scale(m1=H + 1))
    assert "retained rows" in _err(scale(m1=17, H=64))
    assert "NULL" in _err(lib.nps_spectral_film_scale(None, WF, BF, S, B, K, COUT, H, M1, M2, 0, None))
    pb = lambda K=K, mode=0: lib.nps_spectral_film_param_bwd(GS, P, WF, None, None, None, B, K, COUT, H, M1, M2, mode,
                                                            None)
    assert "K" in _err(pb(K=0))
    assert "transform_mode" in _err(pb(mode=3))
    assert "NULL" in _err(lib.nps_spectral_mix_scaled(X, W1, None, Y, B, 4, M2, CIN, COUT, None))
    assert "positive" in _err(lib.nps_spectral_mix_scaled(X, W1, S, Y, 0, 4, M2, CIN, COUT, None))
    assert "NULL" in _err(lib.nps_spectral_film_bwd(Y, S, None, GS, B, 4, M2, COUT, None))


def test_film_composites_check_their_arguments_before_any_launch():
    import nps_hip
    lib = nps_hip.lib

    def fwd(K=K, mode=0, p=P, m2=M2, nchw=False, x_bs=0):
        if nchw:
            return lib.nps_spectral_conv2d_film_fwd_nchw(X, x_bs, W1, W2, p, WF, BF, Y, 0, WS, B, CIN, COUT, H, W, M1,
                                                         m2, K, mode, 0, 0, None)
        return lib.nps_spectral_conv2d_film_fwd(X, W1, W2, p, WF, BF, Y, WS, B, CIN, COUT, H, W, M1, m2, K, mode, 0, 0,
                                                None)

    def bwd(K=K, mode=0, nchw=False, dw2=None):
        if nchw:
            return lib.nps_spectral_conv2d_film_bwd_nchw(X, 0, W1, W2, P, WF, BF, DY, 0, None, 0, 0x9000, dw2, None,
                                                         None, None, WS, B, CIN, COUT, H, W, M1, M2, K, mode, None)
        return lib.nps_spectral_conv2d_film_bwd(X, W1, W2, P, WF, BF, DY, None, 0x9000, dw2, None, None, None, WS, B,
                                                CIN, COUT, H, W, M1, M2, K, mode, None)

    for nchw in (False, True):
        assert "K" in _err(fwd(K=0, nchw=nchw))
        assert "transform_mode" in _err(fwd(mode=2, nchw=nchw))
        assert "NULL" in _err(fwd(p=None, nchw=nchw))
        assert "modes" in _err(fwd(m2=W // 2 + 2, nchw=nchw))
        assert "K" in _err(bwd(K=-1, nchw=nchw))
        assert "transform_mode" in _err(bwd(mode=5, nchw=nchw))
        assert "both" in _err(bwd(nchw=nchw))  # dw1 without dw2
    assert "batch stride" in _err(fwd(nchw=True, x_bs=CIN * H * W - 1))
    assert lib.nps_spectral_conv2d_film_workspace(B, CIN, COUT, H, W, M1, W // 2 + 2) == 0
    assert (lib.nps_spectral_conv2d_film_workspace(B, CIN, COUT, H, W, M1, M2)
            > lib.nps_spectral_conv2d_workspace(B, CIN, COUT, H, W, M1, M2))
