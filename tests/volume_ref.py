"""Plain-torch restatement of approx_volume_preserve_mode 'block' and 'individual' (reference
models/activation_wrapper.py:40-79) on 2-D grids, in whatever dtype the arguments carry, the closed forms the HIP
factor kernels evaluate (csrc/volume.hip), and the synthetic inputs the volume tests share.

Notation: u (B, c, tw, H, W) is the model output after tanh and the optional mask, x_last (B, c, H, W) the last time
step of the model input, s_t = sum_hw u[b,c,t], p = sum_hw x_last[b,c], m = max_pct_dif (a scalar in both modes),
r(s, p) = 1 - tanh((1 - s / p) 100 / m) m / 100.  Every mode is out = u F, then out -= mask out.
"""
import functools

import torch

MODES = ("block", "individual")
MASK_CH = 1
T_IN = 3  # time steps of the model input x: prev_tot reads its last one through a strided view
Z_TARGETS = (-40.0, -3.0, -1.0, -0.3, 0.0, 0.3, 1.0, 3.0, 40.0)
# (B, c, tw, H, W): a ragged 437-element plane with B * c = 9 (one (b, c) per z target in 'block'); a 2115-element
# plane (several blocks per plane); tw = 1; B * c = 65, one past a 64-thread block of the factor kernels, on odd
# 15-element planes
SHAPES = [(3, 3, 25, 19, 23), (1, 1, 4, 47, 45), (9, 2, 1, 5, 7), (13, 5, 3, 3, 5)]
M_VALUES = (1.0, 1.0 / 25.0)


# ------------------------------------------------------------------ the reference's arithmetic, line by line
def forward(u, x_last, m, mode, mask=None, mask_ch=MASK_CH):
    """activation_wrapper.py:40-53 ('block'), :54-79 ('individual'), and the mask re-applied (:104-105)."""
    prev = x_last.sum((2, 3))                                                     # :41 / :60
    if mode == "block":
        mean_tot = u.sum((3, 4)).mean(2)                                          # :42
        dif = torch.tanh((1 - mean_tot / prev) * 100 / m) / 100 * m               # :43-44
        resc = 1 - dif
        v = (u / mean_tot[:, :, None, None, None]) * (prev * resc)[:, :, None, None, None]   # :53
    elif mode == "individual":
        tot = u.sum((3, 4))                                                       # :55
        resc_all, prev_all = torch.zeros_like(tot), torch.zeros_like(tot)
        prev_all[:, :, 0] = prev
        for i in range(tot.shape[-1]):                                            # :62-70
            dif = torch.tanh((1 - tot[:, :, i] / prev) * 100 / m) / 100 * m
            resc = 1 - dif
            resc_all[:, :, i] = resc
            if i < tot.shape[-1] - 1:
                prev_all[:, :, i + 1] = resc * prev
                prev = resc * prev
        v = (u / tot[..., None, None]) * (resc_all * prev_all)[..., None, None]   # :79
    else:
        raise ValueError(f"Unrecognized approx_volume_preserve_mode '{mode}'")
    if mask is not None:
        v = v - mask[:, mask_ch][:, None, None] * v
    return v


# ------------------------------------------------------------------ the closed forms of the factor kernels
def factors(s, p, m, mode):
    """F (B, c, tw) from the totals s (B, c, tw) and p (B, c)."""
    k = 100.0 / m
    if mode == "block":
        sm = s.mean(2)
        r = 1 - torch.tanh((1 - sm / p) * k) / k
        return (p * r / sm)[:, :, None].expand_as(s).clone()
    F = torch.empty_like(s)
    for i in range(s.shape[2]):
        q = (1 - torch.tanh((1 - s[:, :, i] / p) * k) / k) * p
        F[:, :, i] = q / s[:, :, i]
        p = q
    return F


def coefs(s, p, D, m, mode):
    """c (B, c, tw), c_t = sum_t' D_t' dF_t'/ds_t with D_t = sum_hw g (1 - mask) u."""
    k = 100.0 / m
    tw = s.shape[2]
    if mode == "block":
        sm = s.mean(2)
        th = torch.tanh((1 - sm / p) * k)
        r = 1 - th / k
        c = D.sum(2) * ((1 - th * th) / sm - p * r / (sm * sm)) / tw
        return c[:, :, None].expand_as(s).clone()
    ps = []
    for i in range(tw):
        ps.append(p)
        p = (1 - torch.tanh((1 - s[:, :, i] / p) * k) / k) * p
    c = torch.empty_like(s)
    lam = torch.zeros_like(p)
    for i in reversed(range(tw)):
        pi, si, di = ps[i], s[:, :, i], D[:, :, i]
        th = torch.tanh((1 - si / pi) * k)
        r = 1 - th / k
        a = di / si + lam
        c[:, :, i] = -di * r * pi / (si * si) + a * (1 - th * th)
        lam = a * (r - (1 - th * th) * si / pi)
    return c


def backward_closed_form(u, x_last, g, m, mode, mask=None, mask_ch=MASK_CH):
    """gu = g1 F + c with g1 = g (1 - mask): what VolumeModeFn.backward launches, in the dtype of the arguments."""
    g1 = g if mask is None else g - mask[:, mask_ch][:, None, None] * g
    s, p = u.sum((3, 4)), x_last.sum((2, 3))
    D = (g1 * u).sum((3, 4))
    return g1 * factors(s, p, m, mode)[..., None, None] + coefs(s, p, D, m, mode)[..., None, None]


def autograd(u, x_last, g, m, mode, mask, dtype):
    """(output, gradient of u) of `forward` by torch.autograd in `dtype`."""
    uu = u.to(dtype, copy=True).requires_grad_(True)
    y = forward(uu, x_last.to(dtype), m, mode, None if mask is None else mask.to(dtype))
    y.backward(g.to(dtype))
    return y.detach(), uu.grad


# ------------------------------------------------------------------ synthetic inputs
def realised_z(u, x_last, m, mode):
    """|z| (B, c, tw) of the tanh argument each plane (block: each (b, c), repeated over t) meets, in fp64."""
    s, p = u.double().sum((3, 4)), x_last.double().sum((2, 3))
    if mode == "block":
        return ((1 - s.mean(2) / p) * 100 / m).abs()[:, :, None].expand_as(s)
    z = torch.empty_like(s)
    for i in range(s.shape[2]):
        z[:, :, i] = (1 - s[:, :, i] / p) * 100 / m
        p = (1 - torch.tanh(z[:, :, i]) / 100 * m) * p
    return z.abs()


def make_inputs(shape, m, mode, seed, z_targets=Z_TARGETS, premasked=False):
    """fp32 u, x and a two-channel mask (read at channel 1, channel 0 its complement) whose plane totals realise the
    z targets: 'individual' builds them sequentially in fp64, s_i = p_i (1 - z_i m / 100), p_{i+1} = r_i p_i; 'block'
    picks the mean total per (b, c) from the target and spreads it over t with weights in [0.5, 1.5] of mean 1.
    premasked: u is zero on the mask (as the wrapper's first mask application leaves it) and still has those totals."""
    B, c, tw, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, c, T_IN, H, W, generator=g)
    p = x[:, :, -1].double().sum((2, 3))
    u64 = torch.rand(B, c, tw, H, W, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, 2, H, W, generator=g) < 0.3).float()
    mask[:, 0] = 1 - mask[:, 1]  # channel 0 differs everywhere: a wrong channel shows
    if premasked:
        u64 = u64 * (1 - mask[:, MASK_CH].double())[:, None, None]
    zt = torch.tensor(z_targets, dtype=torch.float64)
    if mode == "block":
        # (from the third target on, so that the single (b, c) of a B * c = 1 shape meets the slope of the tanh)
        z = zt[(torch.arange(B * c) + 2) % len(zt)].view(B, c)
        w = 0.5 + torch.rand(B, c, tw, generator=g, dtype=torch.float64)
        w = w / w.mean(2, keepdim=True)
        want = (p * (1 - z * m / 100))[:, :, None] * w
    else:
        z = zt[torch.arange(B * c * tw) % len(zt)].view(B, c, tw)
        want = torch.empty(B, c, tw, dtype=torch.float64)
        for i in range(tw):
            want[:, :, i] = p * (1 - z[:, :, i] * m / 100)
            p = (1 - torch.tanh(z[:, :, i]) / 100 * m) * p
    u = (u64 * (want / u64.sum((3, 4)))[..., None, None]).float()
    return u, x, mask


@functools.lru_cache(maxsize=None)
def case(shape, m, mode, with_mask):
    """The shared case of one (shape, m, mode, mask): fp32 inputs and the fp64 reference output, computed once."""
    B, c, tw, H, W = shape
    u, x, mask = make_inputs(shape, m, mode, seed=1000 * H + W + (7 if m != 1.0 else 0) + (13 if mode == "block" else 0))
    if not with_mask:
        mask = None
    zr = realised_z(u, x[:, :, -1], m, mode)
    if (B * c if mode == "block" else B * c * tw) >= 4:
        # the realised z must populate the linear, transitional and saturated bands, or the slope of the tanh
        # (forward) and the dF/ds term (backward) contribute nothing.  ('block' at B * c = 1 has one z: it is
        # transitional, asserted below.)
        assert (zr < 0.5).any() and ((zr >= 0.5) & (zr <= 3)).any() and (zr > 20).any(), zr
    else:
        assert ((zr >= 0.5) & (zr <= 3)).all(), zr
    ref = forward(u.double(), x[:, :, -1].double(), m, mode, None if mask is None else mask.double())
    return dict(u=u, x=x, mask=mask, ref=ref, m=m, mode=mode)


def upstream(u, kind):
    g = torch.Generator().manual_seed(99)
    r = torch.randn(u.shape, generator=g)
    # correlated with u: only then is D = sum g (1 - mask) u large enough for the c term to carry weight
    return r if kind == "randn" else u + 0.1 * r
