"""Plain-torch restatement of the grid decoders (dec_grid.py: add_delta :8-31, LinearConv :34-55, TimeConv :58-94,
TimeConvDense :97-146, TimeConvLinear :149-195) and of the activation_wrapper's tanh + spatial-cond mask
(activation_wrapper.py:28-35), as functions of a state_dict.  Everything runs in the dtype of its inputs (fp32, or
fp64 for the references of the GPU tests) and is differentiable by torch autograd.

test_decoders_host.py pins it to the reference's own recorded outputs and gradients (tests/golden/decoders_*.pt) at
1e-12; test_gpu_decoders.py uses it as the fp64 reference at the shapes the fixtures do not hold.
"""
import math

import torch
import torch.nn.functional as F

_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}


def add_delta(delta, u, dt, delta_mode="per_step", delta_dt=True):
    """delta, u (B, c, tw, *spatial).  per_step: u_last + cumsum(dt)[t] * delta; all: u_last + dt * delta; none."""
    if not delta_dt:
        dt = 1
    if delta_mode == "none":
        return delta
    tw, nd = delta.shape[2], delta.dim() - 3
    u_last = u[:, :, -1:]
    if delta_mode == "all":
        return u_last + dt * delta
    assert delta_mode == "per_step", delta_mode
    steps = torch.cumsum(torch.ones(1, 1, tw) * dt, dim=2).to(delta)  # the reference's fp32 cumsum, on delta's device
    return u_last + steps.reshape((1, 1, tw) + (1,) * nd) * delta


def swish(x, beta=1.0):
    return x * torch.sigmoid(beta * x)


def timeconvlinear_dim(tw):
    """decoder_input_dim of TimeConvLinear (dec_grid.py:162-164)."""
    return tw * 3 - 1 - math.ceil((tw - 1) / 2) - (1 if tw == 1 else 0)


def timeconv_sizes(hidden, tw):
    """(stride, kernelsize) of TimeConv's first Conv1d (dec_grid.py:71-74)."""
    var = tw + 9
    stride = hidden // var
    return stride, hidden - stride * var + 1


def _pixels(h, C, L):
    """(B, C*L, *spatial) -> (B*N, C, L): every pixel is one sample of the Conv1d chain."""
    return torch.movedim(h, 1, -1).reshape(-1, C, L)


def _unpixels(d, u):
    """(B*N, c, tw) -> (B, c, tw, *spatial)."""
    B, c, tw = u.shape[:3]
    spatial = tuple(u.shape[3:])
    nd = len(spatial)
    return d.reshape((B,) + spatial + (c, tw)).permute(0, nd + 1, nd + 2, *range(1, nd + 1))


def _pointwise(sd, p, x):
    return _CONV[x.dim() - 2](x, sd[p + "weight"], sd[p + "bias"])


def chain(x, w1=None, b1=None, s1=1, act=None, w2=None, b2=None):
    """The per-pixel chain on x (M, C0, L0): Conv1d(stride s1), act, Conv1d, each only if its weight is given."""
    if w1 is not None:
        x = F.conv1d(x, w1, b1, stride=s1)
        if act is not None:
            x = act(x)
    if w2 is not None:
        x = F.conv1d(x, w2, b2)
    return x


def timeconvdense(sd, h, u, dt, delta_mode="per_step", delta_dt=True, p=""):
    c, tw = u.shape[1:3]
    x = _pixels(_pointwise(sd, p + "pre_decoder.", h), c, 3 * tw)
    d = chain(x, sd[p + "decoder.0.weight"], sd[p + "decoder.0.bias"], 2, F.gelu, sd[p + "decoder.2.weight"],
              sd[p + "decoder.2.bias"])
    return add_delta(_unpixels(d, u), u, dt, delta_mode, delta_dt)


def timeconvlinear(sd, h, u, dt, delta_mode="per_step", delta_dt=True, p=""):
    c, tw = u.shape[1:3]
    x = _pixels(_pointwise(sd, p + "pre_decoder.", h), c, timeconvlinear_dim(tw))
    d = chain(x, sd[p + "decoder.weight"], sd[p + "decoder.bias"], 2)
    return add_delta(_unpixels(d, u), u, dt, delta_mode, delta_dt)


def timeconv(sd, h, u, dt, delta_mode="per_step", delta_dt=True, beta=1.0, p=""):
    hidden, tw = h.shape[1], u.shape[2]
    stride, _ = timeconv_sizes(hidden, tw)
    d = chain(_pixels(h, 1, hidden), sd[p + "decoder.0.weight"], sd[p + "decoder.0.bias"], stride,
              lambda z: swish(z, beta), sd[p + "decoder.2.weight"], sd[p + "decoder.2.bias"])
    return add_delta(_unpixels(d, u), u, dt, delta_mode, delta_dt)


def linearconv(sd, h, u, dt, delta_mode="per_step", delta_dt=True, padding_mode="zeros", p=""):
    """'same' conv with an odd kernel: zero or circular padding of (k - 1) / 2 per side."""
    w, b = sd[p + "decoder.weight"], sd[p + "decoder.bias"]
    nd = h.dim() - 2
    pads = [(k - 1) // 2 for k in w.shape[2:]]
    assert all(k % 2 == 1 for k in w.shape[2:])
    if padding_mode == "circular":
        h = F.pad(h, [q for k in reversed(pads) for q in (k, k)], mode="circular")
        d = _CONV[nd](h, w, b)
    else:
        d = _CONV[nd](h, w, b, padding=pads)
    return add_delta(d.reshape(u.shape), u, dt, delta_mode, delta_dt)


DECODERS = dict(TimeConvDense=timeconvdense, TimeConvLinear=timeconvlinear, TimeConv=timeconv, LinearConv=linearconv)


def decoder(cls, sd, h, u, dt, kwargs, p=""):
    """The decoder class `cls` built with the constructor kwargs `kwargs` (those that shape the computation)."""
    kw = dict(delta_mode=kwargs.get("dec_delta_mode", "per_step"), delta_dt=kwargs.get("dec_delta_dt", True), p=p)
    if cls == "LinearConv":
        kw["padding_mode"] = kwargs["dec_padding_mode"]
    if cls == "TimeConv" and "beta" in kwargs:
        kw["beta"] = kwargs["beta"]
    return DECODERS[cls](sd, h, u, dt, **kw)


def wrap(y, final_tanh=False, mask=None):
    """activation_wrapper: tanh, then y - m * y with the mask (B, *spatial) broadcast over (c, tw)."""
    if final_tanh:
        y = torch.tanh(y)
    if mask is not None:
        m = mask[:, None, None].to(y.dtype)
        y = y - m * y
    return y


def reference(fn, tensors, g):
    """fp64: (y, gradients of `tensors` in order) of y = fn(*tensors as fp64 leaves) under the cotangent g."""
    leaves = [t.detach().cpu().double().requires_grad_(True) for t in tensors]
    y = fn(*leaves)
    grads = torch.autograd.grad(y, leaves, g.detach().cpu().double(), allow_unused=True)
    return y.detach(), list(grads)


def reference_sd(fn, sd, h, g):
    """fp64: (y, grad of h, {name: grad}) of y = fn(sd64, h64)."""
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    h64 = h.detach().cpu().double().requires_grad_(True)
    y = fn(sd64, h64)
    keys = list(sd64)
    grads = torch.autograd.grad(y, [h64] + [sd64[k] for k in keys], g.detach().cpu().double())
    return y.detach(), grads[0], dict(zip(keys, grads[1:]))
