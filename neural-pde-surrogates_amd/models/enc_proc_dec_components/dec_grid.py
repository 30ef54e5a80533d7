"""Grid decoders (reference models/enc_proc_dec_components/dec_grid.py).

TimeConvDense with dec_delta_mode='per_step': the pre_decoder 1x1 conv writes a planar (B, 3*c*tw, H, W)
buffer straight from its epilogue; one HIP kernel then runs the per-pixel
Conv1d(k=ceil(tw/2), s=2) -> GELU -> Conv1d chain, add_delta('per_step') and,
when called through activation_wrapper, the final tanh and obstacle mask (nps_timeconv_decode).

Everything else runs on the generic chain kernel (ops.decode_chain, nps_decode_fwd / nps_decode_bwd): TimeConvDense
with 'all' / 'none', TimeConvLinear (one Conv1d stage), TimeConv (Conv1d -> Swish -> Conv1d over the hidden vector
itself, read channels-last), LinearConv (the project's own conv, then the chain with no stage as its add_delta + tanh
+ mask epilogue) and add_delta as a function.  Every decoder has run / run_ad (channels-last h in the grid's flat
frame, as EncProcDec.forward_fused calls them) and forward (the reference's (B, hidden, *spatial) signature).
"""
import math

import numpy as np
import torch
from torch import nn

from models.common import (get_conv_with_right_spatial_dim, Swish, activation_code, use_autograd, flat_frame,
                           run_pointwise)
from nps_hip import ops
from nps_hip import autograd as ad
from pdes import PDE


def dt_cumsum(pde_dt, time_window):
    """fp32 cumsum of (ones(tw) * dt), exactly as dec_grid.py:14-15 builds it."""
    return np.cumsum(np.full(time_window, np.float32(pde_dt), dtype=np.float32), dtype=np.float32)


def _delta_code(delta_mode):
    if delta_mode not in ops.DELTA_MODES:
        raise ValueError(f"Unrecognized dec_delta_mode {delta_mode}")  # dec_grid.py:11, :31
    return ops.DELTA_MODES[delta_mode]


def _chain(spec, x, u, w1=None, b1=None, w2=None, b2=None, dtcum=None, mask=None, train=False):
    """ops.decode_chain, or its differentiable form when `train`."""
    if train:
        return ad.DecodeChainFn.apply(spec, x, u.contiguous(), w1, b1, w2, b2, dtcum, mask)
    det = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    return ops.decode_chain(spec, x, u.contiguous(), det(w1), det(b1), det(w2), det(b2), dtcum, mask)


def add_delta(delta, u, pde_dt, time_window, num_spatial_dims, delta_mode='per_step', delta_dt=True):
    """dec_grid.py:8-31 on device tensors: delta (B, c, tw, *spatial), u the model input -> (B, c, tw, *spatial), as
    the decode chain with no stage (differentiable in delta when it requires grad)."""
    if delta_dt is False:
        pde_dt = 1
    mode = _delta_code(delta_mode)
    if delta.dim() != 3 + num_spatial_dims or tuple(delta.shape) != tuple(u.shape[:2]) + (time_window,) + tuple(u.shape[3:]):
        raise RuntimeError(f"add_delta: delta {tuple(delta.shape)} is not (B, c, time_window={time_window}, *spatial) on "
                           f"the {num_spatial_dims}-D grid of u {tuple(u.shape)}")
    if not delta.is_cuda:
        raise RuntimeError("nps_hip ops run on the MI355X only: tensor is on " + str(delta.device))
    spec = ops.DecodeSpec(planar=True, C0=delta.shape[1], L0=time_window, num_c=delta.shape[1], tw=time_window,
                          delta_mode=mode, dt=float(pde_dt))
    dtcum = torch.from_numpy(dt_cumsum(pde_dt, time_window)).to(delta.device) if mode == 0 else None
    return _chain(spec, delta.contiguous(), u, dtcum=dtcum, train=torch.is_grad_enabled() and delta.requires_grad)


class _GridDecoder(nn.Module):
    """What the grid decoders share: the add_delta constants, the (B, hidden, *spatial) forward around run / run_ad.
    Subclasses set pde, num_c, num_spatial_dims, time_window, dec_delta_mode, dec_delta_dt."""

    def _dt(self):
        return self.pde.dt if self.dec_delta_dt else 1  # dec_grid.py:9-10

    def _dtcum(self, device):
        dt = self._dt()
        key = (float(dt), self.time_window, str(device))
        if getattr(self, "_dt_key", None) != key:
            self._dt_tab = torch.from_numpy(dt_cumsum(dt, self.time_window)).to(device)
            self._dt_key = key
        return self._dt_tab

    def _spec(self, planar, C0, L0, final_tanh, mask_ch, **kw):
        return ops.DecodeSpec(planar=planar, C0=C0, L0=L0, num_c=self.num_c, tw=self.time_window,
                              delta_mode=_delta_code(self.dec_delta_mode), dt=float(self._dt()),
                              act_tanh=bool(final_tanh), mask_ch=mask_ch, **kw)

    def _tab(self, device):
        """The per_step table, for the mode that reads it."""
        return self._dtcum(device) if self.dec_delta_mode == 'per_step' else None

    def _check(self, h, u):
        """Refusals that need no tensor on the device (they come before any launch)."""

    def run_ad(self, h, u, final_tanh=False, mask=None, mask_ch=0):
        """Differentiable form of run()."""
        return self.run(h, u, final_tanh=final_tanh, mask=mask, mask_ch=mask_ch, train=True)

    def forward(self, h: torch.Tensor, u: torch.Tensor, **kwargs):
        """h (B, hidden, *spatial), u (B, c, tw, *spatial) on a 1-D, 2-D or 3-D grid -> (B, c, tw, *spatial)."""
        self._check(h, u)
        if tuple(h.shape[2:]) != tuple(u.shape[3:]) or h.shape[0] != u.shape[0]:
            raise RuntimeError(f"{type(self).__name__}: h {tuple(h.shape)} and u {tuple(u.shape)} lie on different "
                               "grids")
        h = h.reshape((h.shape[0], h.shape[1]) + flat_frame(u.shape[3:]))
        if use_autograd(self):
            return self.run_ad(ad.to_nhwc(h), u)
        return self.run(ops.nchw_to_nhwc(h), u)


class TimeConvDense(_GridDecoder):
    """dec_grid.py:97-146."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, activation,
                 dec_delta_mode='per_step', dec_delta_dt=True, **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.time_window = time_window
        self.num_c = num_c
        self.dec_delta_mode = dec_delta_mode
        self.dec_delta_dt = dec_delta_dt
        decoder_input_dim = time_window * 3 * num_c
        self.pre_decoder = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                                           out_channels=decoder_input_dim, kernel_size=1)
        kernel_size_a = math.ceil(time_window / 2)
        kernel_size_b = math.ceil(time_window / 4) + 1
        if time_window % 4 == 0:
            kernel_size_b += 1
        self.decoder = nn.Sequential(nn.Conv1d(num_c, num_c * 2, kernel_size_a, stride=2),
                                     activation,
                                     nn.Conv1d(num_c * 2, num_c, kernel_size_b, stride=1))

    def _check(self, h=None, u=None):
        if activation_code(self.decoder[1]) != ops.GELU:
            raise NotImplementedError("TimeConvDense: GELU activation only")
        _delta_code(self.dec_delta_mode)

    def _run_chain(self, h, u, final_tanh, mask, mask_ch, train):
        """dec_delta_mode 'all' / 'none': the generic chain kernel (two stages, stride 2, GELU)."""
        c1, c2 = self.decoder[0], self.decoder[2]
        if train:  # the pre-decoder's channels-last output as it is: the chain reads either layout
            pre, planar = self.pre_decoder.run_ad(h), False
        else:
            pre, planar = run_pointwise(self.pre_decoder, [ops.Src(h)], out_nchw=True), True
        spec = self._spec(planar, self.num_c, 3 * self.time_window, final_tanh, mask_ch, s1=2,
                          act=ops.DECODE_ACT_GELU)
        return _chain(spec, pre, u, c1.weight, c1.bias, c2.weight, c2.bias, self._tab(h.device), mask, train)

    def run(self, h, u, final_tanh=False, mask=None, mask_ch=0):
        """h: (B,H,W,hidden) NHWC — a 1-D / 3-D grid's flat pixels as the (B, 1, L, hidden) / (B, D*H, W, hidden)
        view (common.flat_frame); u: model input (B,c,tw,*spatial).  Returns (B,c,tw,*spatial)."""
        self._check()
        if self.dec_delta_mode != 'per_step':
            return self._run_chain(h, u, final_tanh, mask, mask_ch, False)
        pre = run_pointwise(self.pre_decoder, [ops.Src(h)], out_nchw=True)
        c1, c2 = self.decoder[0], self.decoder[2]
        return ops.timeconv_decode(pre, u.contiguous(), c1.weight.detach().contiguous(), c1.bias.detach(),
                                   c2.weight.detach().contiguous(), c2.bias.detach(), self._dtcum(h.device), mask,
                                   mask_ch, final_tanh, self.num_c, self.time_window)

    def run_ad(self, h, u, final_tanh=False, mask=None, mask_ch=0):
        """Differentiable form of run(): pre-decoder conv, planar transpose, fused conv1d-chain kernel."""
        self._check()
        if self.dec_delta_mode != 'per_step':
            return self._run_chain(h, u, final_tanh, mask, mask_ch, True)
        pre = ad.to_nchw(self.pre_decoder.run_ad(h))
        c1, c2 = self.decoder[0], self.decoder[2]
        return ad.TimeConvDecodeFn.apply((mask_ch, bool(final_tanh), self.num_c, self.time_window), pre,
                                         u.contiguous(), c1.weight, c1.bias, c2.weight, c2.bias,
                                         self._dtcum(h.device), mask)


class TimeConvLinear(_GridDecoder):
    """dec_grid.py:149-195: pre_decoder 1x1 conv to num_c x decoder_input_dim per pixel, then one
    Conv1d(num_c -> num_c, k=ceil(tw/2), stride 2) over it (`activation` is accepted and unused, as in the
    reference)."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, activation,
                 dec_delta_mode='per_step', dec_delta_dt=True, **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.time_window = time_window
        self.num_c = num_c
        self.dec_delta_mode = dec_delta_mode
        self.dec_delta_dt = dec_delta_dt
        self.decoder_input_dim = time_window * 3 - 1 - math.ceil((time_window - 1) / 2)
        if time_window == 1:
            self.decoder_input_dim -= 1
        self.pre_decoder = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                                           out_channels=self.decoder_input_dim * num_c,
                                                           kernel_size=1)
        kernel_size_a = math.ceil(time_window / 2)
        self.decoder = nn.Conv1d(num_c, num_c, kernel_size_a, stride=2)

    def run(self, h, u, final_tanh=False, mask=None, mask_ch=0, train=False):
        if train:
            pre, planar = self.pre_decoder.run_ad(h), False
        else:
            pre, planar = run_pointwise(self.pre_decoder, [ops.Src(h)], out_nchw=True), True
        spec = self._spec(planar, self.num_c, self.decoder_input_dim, final_tanh, mask_ch, s1=2)
        return _chain(spec, pre, u, self.decoder.weight, self.decoder.bias, dtcum=self._tab(h.device), mask=mask,
                      train=train)


class TimeConv(_GridDecoder):
    """dec_grid.py:58-94: Conv1d(1 -> 8, kernelsize, stride) -> Swish -> Conv1d(8 -> num_c, 10) over each pixel's
    hidden vector, which the chain kernel reads from the channels-last h itself."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, dec_delta_mode='per_step',
                 dec_delta_dt=True, **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.time_window = time_window
        self.num_c = num_c
        self.dec_delta_mode = dec_delta_mode
        self.dec_delta_dt = dec_delta_dt
        var = time_window + 9
        stride = hidden_features // var
        assert stride > 0, "found stride 0 -- most likely, hidden_features is too small!"
        kernelsize = hidden_features - stride * var + 1
        self.decoder = nn.Sequential(nn.Conv1d(1, 8, kernelsize, stride=stride), Swish(), nn.Conv1d(8, num_c, 10))

    def run(self, h, u, final_tanh=False, mask=None, mask_ch=0, train=False):
        c1, act, c2 = self.decoder[0], self.decoder[1], self.decoder[2]
        if not isinstance(act, Swish):
            raise NotImplementedError(f"TimeConv: the chain kernel applies Swish, not {act!r}")
        spec = self._spec(False, 1, h.shape[-1], final_tanh, mask_ch, s1=c1.stride[0], act=ops.DECODE_ACT_SWISH,
                          beta=float(act.beta))
        return _chain(spec, h if h.is_contiguous() else h.contiguous(), u, c1.weight, c1.bias, c2.weight, c2.bias,
                      self._tab(h.device), mask, train)


class LinearConv(_GridDecoder):
    """dec_grid.py:34-55: one 'same' conv (no activation) to num_c * tw channels on the project's own Conv1d / Conv2d,
    then the chain kernel with no stage as add_delta + tanh + mask on the conv's channels-last output.  2-D: an odd
    dec_kernel_size with zero or circular padding; 1-D: what models.common.Conv1d runs; 3-D: refused."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, dec_kernel_size,
                 dec_padding_mode, dec_delta_mode='per_step', dec_delta_dt=True, **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.time_window = time_window
        self.num_c = num_c
        self.dec_delta_mode = dec_delta_mode
        self.dec_delta_dt = dec_delta_dt
        self.decoder = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                                       out_channels=num_c * time_window, kernel_size=dec_kernel_size,
                                                       padding="same", padding_mode=dec_padding_mode)

    def _check(self, h=None, u=None):
        if self.num_spatial_dims == 3:
            raise NotImplementedError("dec_grid.LinearConv: no 3-D HIP path (1-D and 2-D grids only); the per-pixel "
                                      "decoders TimeConvDense, TimeConvLinear and TimeConv run on 3-D grids")
        if self.num_spatial_dims == 2 and any(k % 2 == 0 for k in self.decoder.kernel_size):
            raise NotImplementedError(f"dec_grid.LinearConv: odd dec_kernel_size only on 2-D grids, got "
                                      f"{tuple(self.decoder.kernel_size)}")

    def run(self, h, u, final_tanh=False, mask=None, mask_ch=0, train=False):
        self._check()
        y = self.decoder.run_ad(h) if train else self.decoder.run([ops.Src(h)], tuple(h.shape[1:3]))
        if tuple(y.shape[:3]) != tuple(h.shape[:3]):
            raise RuntimeError(f"LinearConv: the 'same' conv turned {tuple(h.shape)} into {tuple(y.shape)}")
        spec = self._spec(False, self.num_c, self.time_window, final_tanh, mask_ch)
        return _chain(spec, y if y.is_contiguous() else y.contiguous(), u, dtcum=self._tab(h.device), mask=mask,
                      train=train)
