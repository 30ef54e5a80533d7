"""The 3-D U-Net and 3-D U-FNO train on the GPU: ResidualBlock.run_ad3d, UNetModern.run_ad3d and UFNO.forward in grad
mode against the CPU oracle (oracle.functional residual_block3d / unet_modern3d / ufno3d) in fp64 — complex spectral
weights as complex128 — under a random cotangent.

Criterion: y, dh, dvb rel-L2 < 1e-5 (the project's fp32 bar).  Parameters, the rule of _grads_ok in
tests/test_gpu_backward.py: all gradients as one vector rel-L2 < 1e-5; per tensor rel-L2 < 1e-4, or an error below
1e-5 x the norm of the whole gradient (bias / GroupNorm-affine gradients are sums over every voxel that largely
cancel, and a bias feeding a GroupNorm has an analytically zero gradient that both sides resolve only to rounding
noise).  The reference itself gives every parameter a finite, non-zero gradient at every shape used here (asserted:
88 tensors for the two-level U-Net, 188 / 116 for the two- / one-level U-FNO)."""
import functools

import pytest
import torch
from torch import nn

from oracle import functional as Fo
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
TENSOR_TOL = 1e-4

UNET2 = dict(num_spatial_dims=3, hidden_features=16, cond_mode="concat", norm=True, ch_mults=[1, 2], n_blocks=1,
             use1x1=True, padding_mode="circular")
UNET1 = dict(UNET2, ch_mults=[1], use1x1=False)
FNO = dict(hidden_blocks=2, fno_modes=(3, 4, 3), fno_kernel_size=1, fno_conv_mode="single")
SHAPE2, SHAPE1 = (2, 16, 11, 12, 13), (2, 16, 6, 7, 9)
CASES = {
    "unet2_cond2": ("UNetModern", dict(UNET2, n_cond=2), SHAPE2, 88),
    "unet2_cond4": ("UNetModern", dict(UNET2, n_cond=4), SHAPE2, 88),
    "unet1_k3": ("UNetModern", dict(UNET1, n_cond=2), SHAPE1, None),
    "ufno2": ("UFNO", dict(UNET2, n_cond=2, **FNO), SHAPE2, 188),
    "ufno1": ("UFNO", dict(UNET1, use1x1=True, n_cond=2, **FNO), SHAPE1, 116),
}


def _f64(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double()


def _grads_ok(named_ref, named_got):
    keys = list(named_ref)
    for k in keys:
        assert named_got[k] is not None, f"no gradient for {k}"

    def flat(t):
        t = _f64(t)
        return (torch.view_as_real(t) if t.is_complex() else t).reshape(-1)
    ref = torch.cat([flat(named_ref[k]) for k in keys])
    got = torch.cat([flat(named_got[k]) for k in keys])
    total = torch.linalg.vector_norm(ref).item()
    e_all = torch.linalg.vector_norm(got - ref).item() / total
    bad = []
    for k in keys:
        r, g = flat(named_ref[k]), flat(named_got[k])
        d = torch.linalg.vector_norm(g - r).item()
        e = d / max(torch.linalg.vector_norm(r).item(), 1e-30)
        if not (e < TENSOR_TOL or d < TOL * total):
            bad.append((k, e, d / total))
    print(f"parameter gradients: {len(keys)} tensors, whole-vector rel-L2 {e_all:.2e}, outside the rule: {bad}")
    assert e_all < TOL and not bad, (e_all, bad)


def _model(cls, kw, seed=0):
    import models.enc_proc_dec_components as comps
    torch.manual_seed(seed)
    return getattr(comps, cls)(pde=None, activation=nn.GELU(), **kw).to(DEV)


def _oracle_grads(fn, sd, h, vb, gy):
    """fn(sd64, h64, vb64) in fp64 under the cotangent gy -> (y, dh, dvb, {name: grad})."""
    sd64 = {k: _f64(v).requires_grad_(True) for k, v in sd.items()}
    hd = h.double().requires_grad_(True)
    vd = vb.double().requires_grad_(True) if vb is not None else None
    y = fn(sd64, hd, vd)
    (y * gy.double()).sum().backward()
    grads = {k: v.grad for k, v in sd64.items()}
    for k, g in grads.items():  # the condition the reference itself meets: a usable gradient for every parameter
        assert g is not None and torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all(), k
        assert g.abs().max() > 0, k
    return y.detach(), hd.grad, vd.grad if vd is not None else None, grads


@functools.lru_cache(maxsize=None)
def _case(name):
    """The model, its inputs and the fp64 reference of one CASES entry, built once."""
    cls, kw, shape, ntensors = CASES[name]
    m = _model(cls, kw)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(shape, generator=g)
    vb = torch.rand((shape[0], kw["n_cond"]) + shape[2:], generator=g)
    gy = torch.randn(shape, generator=g)
    sd = {k: v for k, v in m.named_parameters()}
    assert ntensors is None or len(sd) == ntensors
    ofn = Fo.unet_modern3d if cls == "UNetModern" else Fo.ufno3d
    ref = _oracle_grads(lambda s, hh, vv: ofn(s, "", kw, hh, vv), sd, h, vb, gy)
    return m, h, vb, gy, ref


def _zero_grads(m):
    for p in m.parameters():
        p.grad = None


def _compare(m, y, hg, vg, ref, channels_last):
    ry, rdh, rdvb, rgrads = ref
    errs = dict(y=rel_l2(y.permute(0, 4, 1, 2, 3) if channels_last else y, ry), dh=rel_l2(hg.grad, rdh))
    if vg is not None:  # (hg and vg are the channels-first leaves)
        errs["dvb"] = rel_l2(vg.grad, rdvb)
    print(" ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    _grads_ok(rgrads, {k: p.grad for k, p in m.named_parameters()})


# ---------------------------------------------------------------- ResidualBlock.run_ad3d
@pytest.mark.parametrize("pad", [dict(padding_mode="circular"), dict(padding=1)], ids=["valid", "ones"])
def test_residual_block_run_ad3d(pad):
    """16 -> 32 channels (1x1x1 shortcut conv) on (2, ., 6, 7, 9): with padding_mode="circular" the convs are valid,
    so the residual add lands at a positive offset."""
    from models.common import ad_to_ndhwc
    from models.enc_proc_dec_components.proc_unet_modern import ResidualBlock
    from nps_hip import ops
    torch.manual_seed(0)
    m = ResidualBlock(16, 32, activation=nn.GELU(), norm=True, num_spatial_dims=3, padding_kwargs=pad).to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 6, 7, 9, generator=g)
    gy = torch.randn(2, 32, 6, 7, 9, generator=g)
    ref = _oracle_grads(lambda s, hh, _: Fo.residual_block3d(s, "", hh, True, pad), dict(m.named_parameters()), x,
                        None, gy)
    xg = x.to(DEV).requires_grad_(True)
    xh = ad_to_ndhwc(xg)
    y = m.run_ad3d([ops.Src3(xh)], xh.shape[1:4])
    assert y.requires_grad and y.shape == (2, 6, 7, 9, 32)
    (y * gy.to(DEV).permute(0, 2, 3, 4, 1)).sum().backward()
    ry, rdh, _, rgrads = ref
    errs = dict(y=rel_l2(y.permute(0, 4, 1, 2, 3), ry), dx=rel_l2(xg.grad, rdh))
    print(" ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    _grads_ok(rgrads, {k: p.grad for k, p in m.named_parameters()})


# ---------------------------------------------------------------- UNetModern.run_ad3d
@pytest.mark.parametrize("name", ["unet2_cond2", "unet2_cond4", "unet1_k3"])
def test_unet_run_ad3d(name):
    """Two levels at (2, 16, 11, 12, 13) — 11 is the smallest extent a second level admits (11 -> 5 -> valid 3^3 twice);
    the up path runs at 16 / 16 / 18 with the skip zero-padded in and the final crop back to the input size — with
    n_cond = 2 (frames of 18 / 34 / 50 channels: generic kernels) and n_cond = 4 (quad kernels); and one level with
    the final 3^3 conv and a zero-padding crop."""
    from models.common import ad_to_ndhwc
    m, h, vb, gy, ref = _case(name)
    _zero_grads(m)
    hg, vg = h.to(DEV).requires_grad_(True), vb.to(DEV).requires_grad_(True)
    y = m.run_ad3d(ad_to_ndhwc(hg), ad_to_ndhwc(vg))
    assert y.requires_grad and y.shape == (h.shape[0],) + h.shape[2:] + (16,)
    (y * gy.to(DEV).permute(0, 2, 3, 4, 1)).sum().backward()
    _compare(m, y, hg, vg, ref, channels_last=True)


# ---------------------------------------------------------------- UFNO.forward (the public entry)
@pytest.mark.parametrize("name", ["ufno2", "ufno1"])
def test_ufno_forward_trains(name):
    """Grad mode, trainable parameters: forward() hands back a graph, and its gradients match ufno3d's."""
    m, h, vb, gy, ref = _case(name)
    _zero_grads(m)
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    hg, vg = h.to(DEV).requires_grad_(True), vb.to(DEV).requires_grad_(True)
    y = m(hg, variables_broadcast=vg)
    assert y.requires_grad and y.shape == h.shape
    (y * gy.to(DEV)).sum().backward()
    _compare(m, y, hg, vg, ref, channels_last=False)


@pytest.mark.parametrize("name", ["ufno2", "ufno1", "unet2_cond2"])
def test_autograd_forward_equals_inference_forward(name):
    from models.common import to_ndhwc, to_ncdhw, ad_to_ndhwc, ad_to_ncdhw
    m, h, vb, _, _ = _case(name)
    hd, vd = h.to(DEV), vb.to(DEV)
    if name.startswith("ufno"):
        y_ad = m(hd, variables_broadcast=vd)
        with torch.no_grad():
            y_inf = m(hd, variables_broadcast=vd)
    else:
        y_ad = ad_to_ncdhw(m.run_ad3d(ad_to_ndhwc(hd), ad_to_ndhwc(vd)))
        with torch.no_grad():
            y_inf = to_ncdhw(m.run3d(to_ndhwc(hd), to_ndhwc(vd)))
    assert y_ad.requires_grad and not y_inf.requires_grad
    err = rel_l2(y_ad, y_inf)
    print(f"{name}: autograd forward vs inference forward rel-L2 {err:.2e}")
    assert err < TOL


def test_golden_ufno3d_single_through_the_autograd_forward():
    import models.enc_proc_dec_components as comps
    g = load_golden("ufno3d_single")
    kw = dict(g["kwargs"])
    if isinstance(kw.get("fno_modes"), list):
        kw["fno_modes"] = tuple(kw["fno_modes"])
    m = comps.UFNO(pde=None, **kw)
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV)
    y = m(g["h"].to(DEV), variables_broadcast=g["vb"].to(DEV))
    assert y.requires_grad
    assert rel_l2(y, g["y"]) < TOL


def test_one_adam_step():
    m, h, vb, gy, _ = _case("ufno1")
    _zero_grads(m)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    try:
        loss = ((m(h.to(DEV), variables_broadcast=vb.to(DEV)) - gy.to(DEV)) ** 2).mean()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss).item()
        for k, p in m.named_parameters():
            assert torch.isfinite(torch.view_as_real(p) if p.is_complex() else p).all(), k
            assert not torch.equal(p.detach(), before[k]), f"{k} did not move"
    finally:  # the cached model goes back to the parameters its reference was computed with
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(before[k])
        _zero_grads(m)


def test_refusals_and_unchanged_behaviour():
    from models.common import to_ndhwc, to_ncdhw
    m, h, vb, _, _ = _case("ufno1")
    hd, vd = h.to(DEV), vb.to(DEV)
    with pytest.raises(NotImplementedError, match="fp32 for training"):
        m(hd.bfloat16(), variables_broadcast=vd.bfloat16())     # grad mode, trainable parameters, bf16 input
    with torch.no_grad():
        y_inf = m(hd, variables_broadcast=vd)
        assert torch.equal(y_inf, to_ncdhw(m.run3d(to_ndhwc(hd), to_ndhwc(vd))))
    try:
        for p in m.parameters():
            p.requires_grad_(False)
        y = m(hd, variables_broadcast=vd)                       # frozen parameters: the inference path
        assert not y.requires_grad and torch.equal(y, y_inf)
    finally:
        for p in m.parameters():
            p.requires_grad_(True)
    unet = _case("unet2_cond2")[0]
    with pytest.raises(NotImplementedError):                    # the module boundary (run_form) still refuses
        unet(_case("unet2_cond2")[1].to(DEV), variables_broadcast=_case("unet2_cond2")[2].to(DEV))
