"""CPU restatement of EncProcDec on 1-D, 2-D and 3-D grids (enc_proc_dec.py:117-183 with enc_grid.ElementWise,
:41-50, and dec_grid.TimeConvDense, :126-146 + add_delta 'per_step', :8-31), written over the spatial axes: torch.cat,
pointwise F.conv1d / F.conv3d, GELU, the per-pixel Conv1d chain; the processors are oracle.functional's fno3d /
ufno3d / unet_modern3d and the 1-D FNO of tests/spectral1d_ref.py.  It runs in the dtype of its inputs (fp32, or
fp64 with complex128 spectral weights) and is differentiable by torch autograd.

test_encprocdec_nd_host.py pins it to the reference's recorded outputs and gradients (tests/golden/encprocdec_nd.pt);
the GPU tests use it as the reference at the shapes and processors the fixture does not cover.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import functional as Fo
from spectral1d_ref import fno_layer1d_ref

_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
_j = Fo._j  # key prefix ("" = the root) + child name


def pointwise(sd, p, x):
    """A kernel-1 Conv1d / Conv2d / Conv3d with the state_dict's own weight."""
    return _CONV[x.dim() - 2](x, sd[_j(p, "weight")], sd[_j(p, "bias")])


def broadcast_conditioning(cond, spatial_cond, spatial):
    """enc_proc_dec.py:127-137: variables_broadcast (B, K + S, *spatial) or None."""
    vb = None
    if cond is not None:
        vb = cond.reshape(cond.shape[:2] + (1,) * len(spatial)).expand(cond.shape[:2] + tuple(spatial))
    if spatial_cond is not None:
        vb = spatial_cond if vb is None else torch.cat([vb, spatial_cond.to(vb.dtype)], dim=1)
    return vb


def encoder(sd, p, u, pos, vb):
    """enc_grid.py:41-50 with GELU."""
    if pos.dim() == 2:
        pos = pos.unsqueeze(-1)
    h = torch.cat([u.flatten(1, 2), torch.movedim(pos, -1, 1)] + ([vb] if vb is not None else []), dim=1)
    h = F.gelu(pointwise(sd, _j(p, "encoder.0"), h))
    return F.gelu(pointwise(sd, _j(p, "encoder.2"), h))


def decoder(sd, p, h, u, dt, final_tanh=False):
    """dec_grid.py:126-146, then add_delta 'per_step' (:8-31) and the optional activation_wrapper tanh."""
    B, num_c, tw = u.shape[:3]
    spatial = tuple(u.shape[3:])
    nd = len(spatial)
    h = pointwise(sd, _j(p, "pre_decoder"), h)
    h = torch.movedim(h, 1, -1).reshape(-1, num_c, 3 * tw)  # every pixel is one sample of the Conv1d chain
    d = F.gelu(F.conv1d(h, sd[_j(p, "decoder.0.weight")], sd[_j(p, "decoder.0.bias")], stride=2))
    d = F.conv1d(d, sd[_j(p, "decoder.2.weight")], sd[_j(p, "decoder.2.bias")])
    d = d.reshape((B,) + spatial + (num_c, tw)).permute(0, nd + 1, nd + 2, *range(1, nd + 1))
    dts = torch.cumsum(torch.ones(1, 1, tw) * dt, dim=2).to(u.dtype).reshape((1, 1, tw) + (1,) * nd)  # fp32 cumsum
    y = u[:, :, -1:] + dts * d
    return torch.tanh(y) if final_tanh else y


def _fno1d(sd, p, cfg, h, vb):
    for i in range(cfg.get("hidden_blocks", 4)):
        h_in = torch.cat([h, vb], dim=1) if vb is not None else h
        h = fno_layer1d_ref(sd, f"{p}.fno_layers.{i}.", h_in).to(h.dtype)
    return h


def processor(sd, p, name, cfg, nd, h, vb):
    if name == "FNO" and nd == 1:
        return _fno1d(sd, p, cfg, h, vb)
    if nd == 3 and name in ("FNO", "UFNO", "UNetModern"):
        fn = dict(FNO=Fo.fno3d, UFNO=Fo.ufno3d, UNetModern=Fo.unet_modern3d)[name]
        return fn(sd, p, cfg, h, vb)
    raise NotImplementedError(f"{name} in {nd}-D")


def processors_of(cfg):
    """[(class name, merged kwargs)] of cfg["processor"]: a name, a dict(object=...) or a list of either."""
    procs = cfg["processor"] if isinstance(cfg["processor"], (list, tuple)) else [cfg["processor"]]
    base = {k: v for k, v in cfg.items() if k != "processor"}
    out = []
    for pr in procs:
        extra = {} if isinstance(pr, str) else {k: v for k, v in pr.items() if k != "object"}
        out.append((pr if isinstance(pr, str) else pr["object"], dict(base, **extra)))
    return out


def encprocdec_nd(sd, cfg, pde, x, cond=None, pos=None, spatial_cond=None, final_tanh=False):
    """EncProcDec.forward (grid branch) for the model kwargs cfg and the pde numbers pde (dt, n_cond_static,
    n_cond_spatial); sd holds the model's state_dict in x's precision."""
    spatial = tuple(x.shape[3:])
    nd = len(spatial)
    assert nd == cfg["num_spatial_dims"]
    vb = broadcast_conditioning(cond, spatial_cond, spatial)
    n_cond = pde["n_cond_static"] + pde["n_cond_spatial"]
    assert (0 if vb is None else vb.shape[1]) == n_cond
    h = encoder(sd, "encoder", x, pos, vb)
    for i, (name, kw) in enumerate(processors_of(cfg)):
        h_next = processor(sd, f"processor.{i}", name, dict(kw, n_cond=n_cond), nd, h, vb)
        h = h_next + h if (cfg.get("processor_residual", False) and i > 0) else h_next
    return decoder(sd, "decoder", h, x, pde["dt"], final_tanh)


def to_precision(sd, double):
    """The state_dict's tensors (detached, on the CPU) as fp64 / complex128 leaves, or as they are."""
    def conv(t):
        t = t.detach().cpu()
        if double:
            t = t.to(torch.complex128) if t.is_complex() else t.double()
        return t
    return {k: conv(v) for k, v in sd.items()}


def reference_grads(sd, cfg, pde, x, cond, pos, spatial_cond, g, final_tanh=False):
    """fp64: (y, {parameter name: gradient}) of the restatement under the cotangent g."""
    sd64 = {k: v.requires_grad_(True) for k, v in to_precision(sd, True).items()}
    dbl = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    y = encprocdec_nd(sd64, cfg, pde, dbl(x), dbl(cond), dbl(pos), dbl(spatial_cond), final_tanh)
    (y * dbl(g)).sum().backward()
    return y.detach(), {k: v.grad for k, v in sd64.items()}


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """One case of tests/golden/encprocdec_nd.pt with its reference gradients (read-only: shared by the tests)."""
    from conftest import load_golden
    g = dict(load_golden("encprocdec_nd")[name])
    if "grads" not in g:  # the 3-D case's gradients fill a file of their own (the 1 MiB limit per committed file)
        g["grads"] = load_golden("encprocdec_nd_grads3d")[name]
    return g


TOL, TENSOR_TOL = 1e-5, 1e-4


def grads_ok(named_ref, named_got):
    """The parameter-gradient rule of tests/test_gpu_unet3d_train.py (_grads_ok): every tensor has a gradient; all
    gradients as one vector rel-L2 < 1e-5; per tensor rel-L2 < 1e-4, or an error below 1e-5 x the norm of the whole
    gradient."""
    keys = list(named_ref)
    for k in keys:
        assert named_got.get(k) is not None, f"no gradient for {k}"

    def flat(t):
        t = t.detach().cpu()
        t = torch.view_as_real(t.resolve_conj()) if t.is_complex() else t
        return t.double().reshape(-1)
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
