"""GPU parity of the 1-D FNO family on the HIP path (reference proc_fno.py:158-222 SpectralConv1d, :87-155
FNO_Layer, :22-83 FNO), forward and backward: against the reference's recorded vectors (tests/golden/fno1d.pt) and,
at shapes that cross the kernels' tile / chunk boundaries, against the fp64 restatement of spectral1d_ref.py
(pinned to the same fixture by test_spectral1d_host.py) with torch autograd.

Tolerance: fp32 rel-L2 < 1e-5 (the project's bar), complex tensors compared on (re, im).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2
from spectral1d_ref import CASES, build_module, call_module, spectral1d_ref, synthesis

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
K_ = 3  # feature_transform_dim of the cases built here


@functools.lru_cache(maxsize=None)
def _gold():
    return load_golden("fno1d")


def _module(name):
    g = _gold()[name]
    m = build_module(name, g["kwargs"])
    m.load_state_dict(g["state_dict"])
    return m.to(DEV), g


def _leaf(g, key):
    return g[key].to(DEV).requires_grad_(True) if key in g else None


def _check(what, a, b):
    err = rel_l2(a, b)
    print(f"{what}: rel-L2 {err:.3e}")
    assert err < TOL, what


def _check_grads(m, g, what):
    for k, prm in m.named_parameters():
        assert prm.grad is not None, f"{what}: no gradient for {k}"
        _check(f"{what}: d {k}", prm.grad, g["grads"][k])


def _cl(t):
    """(B, C, L) -> channels-last (B, 1, L, C), the layers' internal view."""
    return t.permute(0, 2, 1).unsqueeze(1).contiguous()


def _cf(t):
    return t.squeeze(1).permute(0, 2, 1)


# ------------------------------------------------------------------ the reference's own vectors
@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_module(name):
    """forward on the module's own (B, C, L) tensors, then backward: y, dx, dp / dvb and every parameter gradient."""
    m, g = _module(name)
    x, p, vb = _leaf(g, "x"), _leaf(g, "p"), _leaf(g, "vb")
    y = call_module(name, m, x, p, vb)
    y.backward(g["g"].to(DEV))
    _check(f"{name}: y", y, g["y"])
    _check(f"{name}: dx", x.grad, g["dx"])
    if p is not None:
        _check(f"{name}: dp", p.grad, g["dp"])
    if vb is not None:
        _check(f"{name}: dvb", vb.grad, g["dvb"])
    _check_grads(m, g, name)
    with torch.no_grad():  # the inference route (fused epilogues, no saved tensors)
        dev = lambda k: g[k].to(DEV) if k in g else None
        yi = call_module(name, m, dev("x"), dev("p"), dev("vb"))
    _check(f"{name}: y (no_grad)", yi, g["y"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_channels_last_run_ad_route(name):
    """The route composite models take: channels-last tensors through run_ad."""
    m, g = _module(name)
    x = _cl(g["x"]).to(DEV).requires_grad_(True)
    p = _leaf(g, "p")
    vb = _cl(g["vb"]).to(DEV).requires_grad_(True) if "vb" in g else None
    if name.startswith("fno1d"):
        y = m.run_ad(x, vb, variables=p)
    elif name.startswith("fno_layer1d"):
        y = m.run_ad(x, p=p)
    else:
        y = m.run_ad(x, p)
    y.backward(_cl(g["g"]).to(DEV))
    _check(f"{name}: y", _cf(y), g["y"])
    _check(f"{name}: dx", _cf(x.grad), g["dx"])
    if p is not None:
        _check(f"{name}: dp", p.grad, g["dp"])
    if vb is not None:
        _check(f"{name}: dvb", _cf(vb.grad), g["dvb"])
    _check_grads(m, g, name + " (channels-last)")


@pytest.mark.parametrize("name", ["spectral1d_odd", "spectral1d_odd_tm1"])
@pytest.mark.parametrize("want", ["weights", "input"])
def test_partial_gradients(want, name):
    """nps_hip.autograd.spectral_conv1d / spectral_conv1d_film with only some gradients requested: weights only (x
    and p frozen: no dx, no dp), input only (parameters frozen: dx, dp and no parameter gradient)."""
    from nps_hip import autograd as ad
    m, g = _module(name)
    m.requires_grad_(want == "weights")
    x = _cl(g["x"]).to(DEV).requires_grad_(want == "input")
    p = g["p"].to(DEV).requires_grad_(want == "input") if "p" in g else None
    y = ad.spectral_conv1d(m, x) if p is None else ad.spectral_conv1d_film(m, x, p)
    y.backward(_cl(g["g"]).to(DEV))
    if want == "weights":
        assert x.grad is None and (p is None or p.grad is None)
        _check_grads(m, g, f"{name} (weights only)")
    else:
        assert all(prm.grad is None for prm in m.parameters())
        _check(f"{name}: dx (input only)", _cf(x.grad), g["dx"])
        if p is not None:
            _check(f"{name}: dp (input only)", p.grad, g["dp"])


def test_fixture_through_the_channels_last_run_route():
    """The inference `run` of layers and FNO on (B, 1, L, C) views, the two-source frame of cond_mode concat."""
    from nps_hip import ops
    for name in ("fno_layer1d", "fno_layer1d_double", "fno1d_film", "fno1d_concat"):
        m, g = _module(name)
        x = _cl(g["x"]).to(DEV)
        p = g["p"].to(DEV) if "p" in g else None
        with torch.no_grad():
            if name.startswith("fno1d"):
                y = m.run(x, _cl(g["vb"]).to(DEV) if "vb" in g else None, variables=p)
            else:
                y = m.run([ops.Src(x)], p=p)
        _check(f"{name}: y (run)", _cf(y), g["y"])


@pytest.mark.parametrize("L", [96, 100])
def test_layer_inference_route_on_longer_signals(L):
    """FNO_Layer.run folds L % 32 == 0 signals into 32-point rows for its pointwise convs (L = 100: not folded);
    both against the fp64 restatement, with FiLM and conv_mode 'double'."""
    from models.enc_proc_dec_components.proc_fno import FNO_Layer
    from spectral1d_ref import fno_layer1d_ref
    torch.manual_seed(13)
    m = FNO_Layer(hidden_dim=12, num_spatial_dims=1, modes=7, hidden_dim_out=8, feature_transform=True,
                  feature_transform_dim=K_, conv_mode="double", kernel_size=1)
    x, p = torch.randn(3, 12, L), torch.rand(3, K_)
    ref = fno_layer1d_ref(m.state_dict(), "", x, p)
    m = m.to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV), p.to(DEV))
    _check(f"layer L={L}: y (no_grad)", y, ref)
    _check(f"layer L={L}: y (grad)", m(x.to(DEV), p.to(DEV)), ref)


# ------------------------------------------------------------------ kernel-path shapes
# (B, Cin, Cout, L, m)
KERNEL_SHAPES = {
    # mixer batch tail, NBC = 2, a second input-channel chunk, a partial 64-channel block, one mode past a 32-mode
    # tile; analysis: unaligned quads, the 12-mode tile, several sub-chunks; synthesis: the 128-channel group
    "mix": (17, 34, 68, 300, 33),
    # odd L, m == L//2+1, Cout % 4 != 0 (the VALU mixer, the scalar synthesis store), no channel quads; one work-group
    # per sample adds three sub-chunks (the last a tail) and stores X directly
    "odd": (3, 5, 6, 77, 39),
    # more than 128 channels (a second channel group) and L spanning several sub-chunks with a tail
    "long": (2, 130, 4, 2050, 8),
    # the kernels' own boundaries.  Analysis: 8 slots x 12 modes = 96 modes per pass, so m = 100 takes a second mode
    # pass (aligned quads, C > 64).  Synthesis: m > 64 switches to 64-channel groups (Cin = 68: a second group in
    # dx) and m = 100 is 6 full 16-mode twiddle passes and a tail
    "modes": (1, 68, 8, 260, 100),
    # the analysis keeps 256-point sub-chunks only when the grid stays >= 512 work-groups (B = 512), and the
    # synthesis then walks several tiles per work-group, ending inside the run (L = 300 < 8 x 128)
    "batch": (512, 4, 4, 300, 3),
}
VARIANTS = ["plain", "tm0", "tm1"]


@functools.lru_cache(maxsize=None)
def _kernel_case(kind, variant):
    """Module, inputs and the fp64 autograd reference of one case (computed once on the CPU, shared)."""
    from models.enc_proc_dec_components.proc_fno import SpectralConv1d
    B, Cin, Cout, L, m_ = KERNEL_SHAPES[kind]
    film = variant != "plain"
    torch.manual_seed(11)
    m = SpectralConv1d(Cin, Cout, (m_,), feature_transform=film, feature_transform_dim=K_,
                       transform_mode=int(variant[-1]) if film else 1)
    x = torch.randn(B, Cin, L)
    p = torch.rand(B, K_) if film else None
    g = torch.randn(B, Cout, L)
    lx, lw = x.clone().requires_grad_(True), m.weights1.detach().clone().requires_grad_(True)
    if film:
        lp, lWf, lbf = (t.detach().clone().requires_grad_(True) for t in
                        (p, m.weights_feat.weight, m.weights_feat.bias))
        y = spectral1d_ref(lx, lw, (lp, lWf, lbf, m.transform_mode))
    else:
        y = spectral1d_ref(lx, lw)
    y.backward(g.double())
    ref = dict(y=y.detach(), dx=lx.grad, dw=lw.grad)
    if film:
        ref.update(dp=lp.grad, dwf=lWf.grad, dbf=lbf.grad)
    return m, x, p, g, ref


def _run_module(m, x, p, g):
    m = m.to(DEV)
    m.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    pd = p.to(DEV).requires_grad_(True) if p is not None else None
    y = m(xd, pd)
    y.backward(g.to(DEV))
    out = dict(y=y.detach(), dx=xd.grad, dw=m.weights1.grad)
    if p is not None:
        out.update(dp=pd.grad, dwf=m.weights_feat.weight.grad, dbf=m.weights_feat.bias.grad)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", list(KERNEL_SHAPES))
def test_kernel_paths_against_the_fp64_restatement(kind, variant):
    m, x, p, g, ref = _kernel_case(kind, variant)
    got = _run_module(m, x, p, g)
    assert set(got) == set(ref)
    for k in ref:
        _check(f"{kind}/{variant}: {k}", got[k], ref[k])


def test_forward_and_backward_are_bit_repeatable():
    """The analysis sums its partials in a fixed order and nothing uses atomics: the same inputs, the same bits."""
    m, x, p, g, _ = _kernel_case("long", "tm0")
    a = _run_module(m, x, p, g)
    a = {k: v.clone() for k, v in a.items()}
    b = _run_module(m, x, p, g)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ stages
def test_two_sources_equal_the_concatenated_source_bit_for_bit():
    from nps_hip import ops
    torch.manual_seed(3)
    h = torch.randn(2, 300, 6, device=DEV)
    vb = torch.randn(2, 300, 3, device=DEV)
    two = ops.spectral1d_dft([ops.Src(h), ops.Src(vb)], 33)
    one = ops.spectral1d_dft([ops.Src(torch.cat([h, vb], dim=2).contiguous())], 33)
    assert two.shape == (2, 33, 9)
    assert torch.equal(torch.view_as_real(two), torch.view_as_real(one))
    # and with 4-aligned sources (the 16-B load path) against the unaligned path's arithmetic
    h4, vb4 = torch.randn(2, 300, 8, device=DEV), torch.randn(2, 300, 4, device=DEV)
    two = ops.spectral1d_dft([ops.Src(h4), ops.Src(vb4)], 33)
    one = ops.spectral1d_dft([ops.Src(torch.cat([h4, vb4], dim=2).contiguous())], 33)
    assert torch.equal(torch.view_as_real(two), torch.view_as_real(one))


@pytest.mark.parametrize("Cout", [6, 68])
def test_synthesis_epilogues(Cout):
    """accumulate, addend and act = GELU of spectral1d_idft against torch (scalar and 16-B stores)."""
    from nps_hip import ops
    B, L, m = 3, 77, 39
    torch.manual_seed(5)
    Z = torch.randn(B, m, Cout, dtype=torch.complex64)
    base = torch.randn(B, L, Cout)
    add = torch.randn(B, L, Cout)
    y = synthesis(Z.to(torch.complex128), L).permute(0, 2, 1)  # (B, L, Cout) fp64
    Zd = Z.to(DEV)
    _check("plain", ops.spectral1d_idft(Zd, L), y)
    out = base.to(DEV).clone()
    assert ops.spectral1d_idft(Zd, L, out=out, accumulate=True) is out
    _check("accumulate", out, base.double() + y)
    out = base.to(DEV).clone()
    ops.spectral1d_idft(Zd, L, out=out, accumulate=False, addend=add.to(DEV))
    _check("addend", out, y + add.double())
    out = base.to(DEV).clone()
    ops.spectral1d_idft(Zd, L, out=out, accumulate=True, addend=add.to(DEV), act=ops.GELU)
    _check("accumulate + addend + GELU", out, F.gelu(base.double() + y + add.double()))
    _check("GELU", ops.spectral1d_idft(Zd, L, act=ops.GELU), F.gelu(y))


def test_analysis_adjoint_flag():
    """adjoint = 1 scales bin k by c_k / L: the transpose of the synthesis, checked as <idft(Z), g> == <Z, dft_adj(g)>
    through the fp64 synthesis' autograd."""
    from nps_hip import ops
    for L, m in ((300, 33), (77, 39), (8, 5)):
        torch.manual_seed(9)
        g = torch.randn(2, L, 5)
        Z = torch.zeros(2, m, 5, dtype=torch.complex128, requires_grad=True)
        (synthesis(Z, L).permute(0, 2, 1) * g.double()).sum().backward()
        _check(f"adjoint L={L}", ops.spectral1d_dft([ops.Src(g.to(DEV))], m, adjoint=True), Z.grad)


# ------------------------------------------------------------------ the one-call composites, through ctypes only
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("variant", VARIANTS)
def test_composites_through_ctypes(variant):
    import nps_hip
    lib = nps_hip.lib
    m, x, p, g, ref = _kernel_case("mix", variant)
    B, Cin, Cout, L, m_ = KERNEL_SHAPES["mix"]
    film = variant != "plain"
    xl = x.permute(0, 2, 1).contiguous().to(DEV)
    gl = g.permute(0, 2, 1).contiguous().to(DEV)
    w = m.weights1.detach().to(DEV).contiguous()
    y = torch.empty(B, L, Cout, device=DEV)
    dx = torch.empty(B, L, Cin, device=DEV)
    dw = torch.empty_like(w)
    n = (lib.nps_spectral_conv1d_film_workspace if film else lib.nps_spectral_conv1d_workspace)(B, Cin, Cout, L, m_)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    if film:
        pd = p.to(DEV)
        Wf, bf = m.weights_feat.weight.detach().to(DEV).contiguous(), m.weights_feat.bias.detach().to(DEV).contiguous()
        dp, dWf, dbf = torch.empty_like(pd), torch.empty_like(Wf), torch.empty_like(bf)
        mode = int(m.transform_mode)
        rc = lib.nps_spectral_conv1d_film_fwd(_ptr(xl), _ptr(w), _ptr(pd), _ptr(Wf), _ptr(bf), _ptr(y), _ptr(ws), B,
                                              Cin, Cout, L, m_, K_, mode, 0, 0, s)
        assert rc == 0, lib.nps_last_error()
        rc = lib.nps_spectral_conv1d_film_bwd(_ptr(xl), _ptr(w), _ptr(pd), _ptr(Wf), _ptr(bf), _ptr(gl), _ptr(dx),
                                              _ptr(dw), _ptr(dp), _ptr(dWf), _ptr(dbf), _ptr(ws), B, Cin, Cout, L, m_,
                                              K_, mode, s)
        assert rc == 0, lib.nps_last_error()
    else:
        rc = lib.nps_spectral_conv1d_fwd(_ptr(xl), _ptr(w), _ptr(y), _ptr(ws), B, Cin, Cout, L, m_, 0, 0, s)
        assert rc == 0, lib.nps_last_error()
        rc = lib.nps_spectral_conv1d_bwd(_ptr(xl), _ptr(w), _ptr(gl), _ptr(dx), _ptr(dw), _ptr(ws), B, Cin, Cout, L,
                                         m_, s)
        assert rc == 0, lib.nps_last_error()
    torch.cuda.synchronize()
    _check("y", y.permute(0, 2, 1), ref["y"])
    _check("dx", dx.permute(0, 2, 1), ref["dx"])
    _check("dw", dw, ref["dw"])
    if film:
        _check("dp", dp, ref["dp"])
        _check("dwf", dWf, ref["dwf"])
        _check("dbf", dbf, ref["dbf"])
    # accumulate + GELU of the forward composite: y <- GELU(y + conv(x))
    y2 = y.clone()
    if film:
        rc = lib.nps_spectral_conv1d_film_fwd(_ptr(xl), _ptr(w), _ptr(pd), _ptr(Wf), _ptr(bf), _ptr(y2), _ptr(ws), B,
                                              Cin, Cout, L, m_, K_, mode, 1, 1, s)
    else:
        rc = lib.nps_spectral_conv1d_fwd(_ptr(xl), _ptr(w), _ptr(y2), _ptr(ws), B, Cin, Cout, L, m_, 1, 1, s)
    assert rc == 0, lib.nps_last_error()
    _check("GELU(y + y)", y2.permute(0, 2, 1), F.gelu(2 * ref["y"]))
