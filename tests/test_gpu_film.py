"""GPU parity of FiLM conditioning (reference proc_fno.py:271-284) on the HIP path: SpectralConv2d / FNO_Layer / FNO
with feature_transform, forward and backward, against the reference's recorded vectors (tests/golden/film.pt) and,
at shapes that reach the mixer paths the fixture misses, against the fp64 restatement of test_film_host.py (pinned
there to the same fixture) with torch autograd.

Tolerance: fp32 rel-L2 < 1e-5 (the project's bar), complex gradients compared on (re, im).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2
from test_film_host import SPECTRAL, build_module, case_ref, film_scale_ref, film_spectral_ref

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _film():
    return load_golden("film")


def _module(name):
    g = _film()[name]
    m = build_module(name, g["kwargs"])
    m.load_state_dict(g["state_dict"])
    return m.to(DEV), g


def _check_grads(m, g, what):
    for k, prm in m.named_parameters():
        assert prm.grad is not None, f"{what}: no gradient for {k}"
        err = rel_l2(prm.grad, g["grads"][k])
        print(f"{what}: d {k} rel-L2 {err:.3e}")
        assert err < TOL, f"{what}: d {k}"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ the reference's own vectors
@pytest.mark.parametrize("name", SPECTRAL + ["fno_layer", "fno"])
def test_fixture_through_the_module(name):
    """forward(x, p) on the module's own NCHW tensors, then backward: y, dx, dp and every parameter gradient."""
    m, g = _module(name)
    x = g["x"].to(DEV).requires_grad_(True)
    p = g["p"].to(DEV).requires_grad_(True)
    y = m(x, variables=p) if name == "fno" else m(x, p)
    y.backward(g["g"].to(DEV))
    for what, a, b in (("y", y, g["y"]), ("dx", x.grad, g["dx"]), ("dp", p.grad, g["dp"])):
        err = rel_l2(a, b)
        print(f"{name}: {what} rel-L2 {err:.3e}")
        assert err < TOL, what
    _check_grads(m, g, name)
    with torch.no_grad():  # the inference route (fused kernels, no saved tensors)
        yi = m(g["x"].to(DEV), variables=g["p"].to(DEV)) if name == "fno" else m(g["x"].to(DEV), g["p"].to(DEV))
    assert rel_l2(yi, g["y"]) < TOL


@pytest.mark.parametrize("name", SPECTRAL + ["fno_layer", "fno"])
def test_fixture_through_the_nhwc_run_ad_route(name):
    """The route composite models take: NHWC tensors through run_ad / the NHWC autograd function."""
    from nps_hip import autograd as ad
    m, g = _module(name)
    x = _nhwc(g["x"]).to(DEV).requires_grad_(True)
    p = g["p"].to(DEV).requires_grad_(True)
    if name == "fno":
        y = m.run_ad(x, None, variables=p)
    elif name == "fno_layer":
        y = m.run_ad(x, p=p)
    else:
        y = ad.spectral_conv2d_film(m, x, p)
    y.backward(_nhwc(g["g"]).to(DEV))
    assert rel_l2(y.permute(0, 3, 1, 2), g["y"]) < TOL
    assert rel_l2(x.grad.permute(0, 3, 1, 2), g["dx"]) < TOL
    assert rel_l2(p.grad, g["dp"]) < TOL
    _check_grads(m, g, name + " (NHWC)")


@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("want", ["weights", "input"])
def test_partial_gradients_on_the_overlap_fixture(want, nchw):
    """nps_hip.autograd.spectral_conv2d_film(_nchw) with only some gradients requested: weights only (weights1/2 and
    weights_feat; x and p frozen: no dx, no dp), input only (parameters frozen: dx, dp and no parameter gradient)."""
    from nps_hip import autograd as ad
    name = "spectral2d_overlap_tm1"
    m, g = _module(name)
    m.requires_grad_(want == "weights")
    lay = (lambda t: t) if nchw else _nhwc
    x = lay(g["x"]).to(DEV).requires_grad_(want == "input")
    p = g["p"].to(DEV).requires_grad_(want == "input")
    fn = ad.spectral_conv2d_film_nchw if nchw else ad.spectral_conv2d_film
    fn(m, x, p).backward(lay(g["g"]).to(DEV))
    if want == "weights":
        assert x.grad is None and p.grad is None
        _check_grads(m, g, f"{name} (weights only)")
    else:
        assert all(prm.grad is None for prm in m.parameters())
        assert rel_l2(x.grad if nchw else x.grad.permute(0, 3, 1, 2), g["dx"]) < TOL
        assert rel_l2(p.grad, g["dp"]) < TOL


# ------------------------------------------------------------------ mixer paths the fixture misses
H_, W_, M1_, M2_ = 8, 10, 3, 4
# (B, Cin, Cout, K): MFMA mixer with NBC = 2, a batch tail, a second input-channel chunk and a partial second
# 64-channel block; the VALU mixer (Cout % 4 != 0) with a second batch pass (B > 8); K = 1
MIX_SHAPES = {"mfma": (17, 34, 68, 5), "valu": (9, 5, 6, 5), "k1": (17, 34, 68, 1)}


@functools.lru_cache(maxsize=None)
def _mix_case(kind, mode):
    """Module, inputs and the fp64 autograd reference of one mixer-path case (computed once, shared)."""
    from models.enc_proc_dec_components.proc_fno import SpectralConv2d
    B, Cin, Cout, K = MIX_SHAPES[kind]
    torch.manual_seed(7)
    m = SpectralConv2d(Cin, Cout, (M1_, M2_), feature_transform=True, feature_transform_dim=K, transform_mode=mode)
    x = torch.randn(B, Cin, H_, W_)
    p = torch.rand(B, K)
    g = torch.randn(B, Cout, H_, W_)
    leaves = [t.detach().clone().requires_grad_(True) for t in
              (x, m.weights1, m.weights2, p, m.weights_feat.weight, m.weights_feat.bias)]
    y = film_spectral_ref(*leaves, mode)
    y.backward(g.double())
    ref = dict(y=y.detach(), dx=leaves[0].grad, dw1=leaves[1].grad, dw2=leaves[2].grad, dp=leaves[3].grad,
               dwf=leaves[4].grad, dbf=leaves[5].grad)
    return m, x, p, g, ref


def _run_module(m, x, p, g):
    m = m.to(DEV)
    m.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    pd = p.to(DEV).requires_grad_(True)
    y = m(xd, pd)
    y.backward(g.to(DEV))
    return dict(y=y.detach(), dx=xd.grad, dw1=m.weights1.grad, dw2=m.weights2.grad, dp=pd.grad,
                dwf=m.weights_feat.weight.grad, dbf=m.weights_feat.bias.grad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", list(MIX_SHAPES))
def test_mixer_paths_vs_fp64_autograd(kind, mode):
    m, x, p, g, ref = _mix_case(kind, mode)
    got = _run_module(m, x, p, g)
    for k, r in ref.items():
        err = rel_l2(got[k], r)
        print(f"{kind} tm{mode}: {k} rel-L2 {err:.3e}")
        assert err < TOL, k


def test_backward_is_bit_repeatable():
    """The FiLM parameter gradients are fixed-order fp64 sums: two runs give the same bits."""
    m, x, p, g, _ = _mix_case("mfma", 0)
    a = _run_module(m, x, p, g)
    a = {k: v.clone() for k, v in a.items()}
    b = _run_module(m, x, p, g)
    for k in ("dp", "dwf", "dbf"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ stages through ctypes
def _lib():
    from nps_hip import lib
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    if rc != 0:
        raise AssertionError(f"{what}: rc {rc}: {_lib().nps_last_error().decode()}")


def _ws(nbytes):
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)


def _rows(H, m1):
    R = min(H, 2 * m1)
    return [r if r < m1 else H - R + r for r in range(R)]


# overlap (2 m1 > H, the fixture's shape); two 64-channel blocks with more batches than waves, no overlap; m1 == H,
# where every row lies in both corners
@pytest.mark.parametrize("B,K,Cout,H,m1,m2", [(2, 3, 4, 6, 4, 3), (17, 5, 68, 8, 3, 4), (3, 2, 5, 4, 4, 2)])
@pytest.mark.parametrize("mode", [0, 1])
def test_scale_stage_alone(mode, B, K, Cout, H, m1, m2):
    """nps_spectral_film_scale against the closed form of S, so a wrong row map cannot hide behind a small output."""
    torch.manual_seed(11)
    N = Cout * 2 * m1 * m2
    p, Wf, bf = torch.rand(B, K), torch.randn(N, K), torch.randn(N)
    R = min(H, 2 * m1)
    S = torch.full((B, R, m2, Cout), float("nan"), device=DEV)
    pd, wd, bd = p.to(DEV), Wf.to(DEV), bf.to(DEV)
    _ok(_lib().nps_spectral_film_scale(_p(pd), _p(wd), _p(bd), _p(S), B, K, Cout, H, m1, m2, mode, _s()), "film_scale")
    torch.cuda.synchronize()
    ref = film_scale_ref(p, Wf, bf, Cout, H, m1, m2, mode)[:, :, _rows(H, m1)].permute(0, 2, 3, 1)  # (B, R, m2, Cout)
    err = rel_l2(S, ref)
    print(f"film_scale tm{mode} B{B} K{K} Cout{Cout} H{H} m{m1},{m2}: rel-L2 {err:.3e}")
    assert err < TOL
    # every row on its own: a swapped pair of rows cannot average out
    for r in range(R):
        assert rel_l2(S[:, r], ref[:, r]) < TOL, f"row {r}"


@pytest.mark.parametrize("kind", ["mfma", "valu"])
def test_mix_scaled_with_unit_scale_is_mix_bit_for_bit(kind):
    lib = _lib()
    B, Cin, Cout, _ = MIX_SHAPES[kind]
    R, m2 = 2 * M1_, M2_
    torch.manual_seed(3)
    X2 = torch.randn(B, R, m2, Cin, dtype=torch.complex64).to(DEV)
    wp = torch.randn(R, m2, Cin, Cout, dtype=torch.complex64).to(DEV)
    S = torch.ones(B, R, m2, Cout, device=DEV)
    Ya = torch.empty(B, R, m2, Cout, dtype=torch.complex64, device=DEV)
    Yb = torch.empty_like(Ya)
    _ok(lib.nps_spectral_mix(_p(X2), _p(wp), _p(Ya), B, R, m2, Cin, Cout, _s()), "mix")
    _ok(lib.nps_spectral_mix_scaled(_p(X2), _p(wp), _p(S), _p(Yb), B, R, m2, Cin, Cout, _s()), "mix_scaled")
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(Ya), torch.view_as_real(Yb))
    # and a non-trivial S is the elementwise product
    S2 = torch.randn(B, R, m2, Cout, device=DEV)
    _ok(lib.nps_spectral_mix_scaled(_p(X2), _p(wp), _p(S2), _p(Yb), B, R, m2, Cin, Cout, _s()), "mix_scaled")
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(Yb), torch.view_as_real(Ya) * S2[..., None])


# ------------------------------------------------------------------ fused synthesis
def test_film_layer_takes_the_fused_synthesis(monkeypatch):
    """A FiLM FNO_Layer whose shape satisfies spectral_fusable hands Z to its 1x1 `w` (one output pass), in
    inference mode: act(film_spectral(x, p) + w(x))."""
    from nps_hip import ops
    from models.enc_proc_dec_components.proc_fno import FNO_Layer, SpectralConv2d
    B, C, H, W, K = 2, 8, 8, 128, 3
    assert ops.spectral_fusable(W, 4, C)
    torch.manual_seed(5)
    m = FNO_Layer(hidden_dim=C, num_spatial_dims=2, modes=(3, 4), feature_transform=True, feature_transform_dim=K)
    x, p = torch.randn(B, C, H, W), torch.rand(B, K)
    c = m.conv
    ref = F.gelu(film_spectral_ref(x, c.weights1.detach(), c.weights2.detach(), p, c.weights_feat.weight.detach(),
                                   c.weights_feat.bias.detach(), 0)
                 + F.conv2d(x.double(), m.w.weight.detach().double(), m.w.bias.detach().double()))

    def unfused(*a, **k):
        raise AssertionError("the FiLM layer left the fused route (SpectralConv2d.run called)")

    monkeypatch.setattr(SpectralConv2d, "run", unfused)
    m = m.to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV), p.to(DEV))
    err = rel_l2(y, ref)
    print(f"fused FiLM layer: rel-L2 {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------ the one-call ABI, ctypes only
def _film_abi(g, nchw, y0=None, accumulate=0, act=0, sliced=False):
    """nps_spectral_conv2d_film_fwd(_nchw) and _bwd(_nchw) on a fixture case; returns NCHW CPU tensors."""
    lib = _lib()
    sd, kw = g["state_dict"], g["kwargs"]
    x, p, gy = g["x"], g["p"], g["g"]
    B, Cin, H, W = x.shape
    Cout, (m1, m2), K, mode = kw["out_channels"], kw["modes"], kw["feature_transform_dim"], kw["transform_mode"]
    to = (lambda t: t.contiguous().to(DEV)) if nchw else (lambda t: _nhwc(t).to(DEV))
    w1, w2 = sd["weights1"].contiguous().to(DEV), sd["weights2"].contiguous().to(DEV)
    wf, bf, pd = sd["weights_feat.weight"].to(DEV), sd["weights_feat.bias"].to(DEV), p.to(DEV)
    x_bs = 0
    if sliced:  # x as channels [1, 1 + Cin) of a wider tensor: its batch stride is that tensor's
        big = torch.full((B, Cin + 3, H, W), float("nan"), device=DEV)
        big[:, 1:1 + Cin] = x.to(DEV)
        xd, x_bs = big[:, 1:1 + Cin], big.stride(0)
    else:
        xd = to(x)
    yd = to(y0) if y0 is not None else torch.full_like(to(gy), float("nan"))
    gd = to(gy)
    ws = _ws(lib.nps_spectral_conv2d_film_workspace(B, Cin, Cout, H, W, m1, m2))
    dx = torch.full((B, Cin, H, W) if nchw else (B, H, W, Cin), float("nan"), device=DEV)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    dp, dwf, dbf = torch.empty_like(pd), torch.empty_like(wf), torch.empty_like(bf)
    dims = (B, Cin, Cout, H, W, m1, m2, K, mode)
    if nchw:
        _ok(lib.nps_spectral_conv2d_film_fwd_nchw(_p(xd), x_bs, _p(w1), _p(w2), _p(pd), _p(wf), _p(bf), _p(yd), 0,
                                                  _p(ws), *dims, accumulate, act, _s()), "film_fwd_nchw")
        _ok(lib.nps_spectral_conv2d_film_bwd_nchw(_p(xd), x_bs, _p(w1), _p(w2), _p(pd), _p(wf), _p(bf), _p(gd), 0,
                                                  _p(dx), 0, _p(dw1), _p(dw2), _p(dp), _p(dwf), _p(dbf), _p(ws),
                                                  *dims, _s()), "film_bwd_nchw")
    else:
        _ok(lib.nps_spectral_conv2d_film_fwd(_p(xd), _p(w1), _p(w2), _p(pd), _p(wf), _p(bf), _p(yd), _p(ws), *dims,
                                             accumulate, act, _s()), "film_fwd")
        _ok(lib.nps_spectral_conv2d_film_bwd(_p(xd), _p(w1), _p(w2), _p(pd), _p(wf), _p(bf), _p(gd), _p(dx), _p(dw1),
                                             _p(dw2), _p(dp), _p(dwf), _p(dbf), _p(ws), *dims, _s()), "film_bwd")
    torch.cuda.synchronize()
    back = (lambda t: t.cpu()) if nchw else (lambda t: t.permute(0, 3, 1, 2).cpu())
    return dict(y=back(yd), dx=back(dx), dw1=dw1.cpu(), dw2=dw2.cpu(), dp=dp.cpu(), dwf=dwf.cpu(), dbf=dbf.cpu())


def _check_abi(got, g):
    want = dict(y=g["y"], dx=g["dx"], dp=g["dp"], dw1=g["grads"]["weights1"], dw2=g["grads"]["weights2"],
                dwf=g["grads"]["weights_feat.weight"], dbf=g["grads"]["weights_feat.bias"])
    for k, r in want.items():
        err = rel_l2(got[k], r)
        print(f"  {k}: rel-L2 {err:.3e}")
        assert err < TOL, k


@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("mode", [0, 1])
def test_one_call_abi_on_the_overlap_fixture(mode, nchw):
    g = _film()[f"spectral2d_overlap_tm{mode}"]
    _check_abi(_film_abi(g, nchw), g)


def test_one_call_abi_nchw_channel_slice_with_batch_stride():
    g = _film()["spectral2d_overlap_tm0"]
    _check_abi(_film_abi(g, True, sliced=True), g)


@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
def test_one_call_abi_accumulate_and_gelu(nchw):
    """accumulate = 1, act = 1: y = gelu(y + FiLM spectral conv), FNO_Layer's tail."""
    g = _film()["spectral2d_overlap_tm1"]
    torch.manual_seed(9)
    y0 = torch.randn_like(g["y"])
    got = _film_abi(g, nchw, y0=y0, accumulate=1, act=1)
    ref = F.gelu(y0.double() + case_ref("spectral2d_overlap_tm1", g))
    assert rel_l2(got["y"], ref) < TOL
