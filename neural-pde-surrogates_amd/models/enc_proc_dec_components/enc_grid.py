"""Grid encoders (reference models/enc_proc_dec_components/enc_grid.py)."""
import torch
from torch import nn

from models.common import (get_conv_with_right_spatial_dim, Swish, activation_code, use_autograd, Conv2d, flat_frame,
                           run_pointwise)
from nps_hip import ops
from nps_hip import autograd as ad
from pdes import PDE


class LinearConv(nn.Module):
    """enc_grid.py:7-21 — parameters only (not used by the twophase cfgs)."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, enc_kernel_size,
                 enc_padding_mode, **kwargs):
        super().__init__()
        self.encoder = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=num_c * time_window,
                                                       out_channels=hidden_features, kernel_size=enc_kernel_size,
                                                       padding="same", padding_mode=enc_padding_mode)

    def forward(self, u, **kwargs):
        raise NotImplementedError("enc_grid.LinearConv is not on the MI355X path")


class ElementWise(nn.Module):
    """enc_grid.py:24-50: cat(u, pos, vb) -> 1x1 -> act -> 1x1 -> act, two fused HIP launches."""

    def __init__(self, pde: PDE, num_c, num_spatial_dims, time_window, hidden_features, n_cond, activation=Swish(),
                 **kwargs):
        super().__init__()
        num_channels = num_c * time_window
        self.n_in = num_channels + num_spatial_dims + n_cond
        self.encoder = nn.Sequential(
            get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=num_channels + num_spatial_dims + n_cond,
                                            out_channels=hidden_features, kernel_size=1),
            activation,
            get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                            out_channels=hidden_features, kernel_size=1),
            activation,
        )

    def run_packed(self, xin, carry_stats=None):
        """xin: (B,H,W,Cp) NHWC packed [u | pos | vb | 0-pad] (nps_pack_grid_input); a 1-D / 3-D grid's flat pixels
        as the (B, 1, L, Cp) / (B, D*H, W, Cp) view (common.flat_frame).  carry_stats: whether the output carries
        its GroupNorm(1) moments — by default on 2-D grids, where every processor's frames look for them; off them
        the caller asks when a U-Net's first norm will read them (an FNO never does)."""
        act = activation_code(self.encoder[1])
        c1, c2 = self.encoder[0], self.encoder[2]
        # xin carries <= 3 zero channels of padding; the packed weight is zero-padded to
        # 16-channel chunks, so the same packed buffer serves (ceil16(Cp) == ceil16(n_in)).
        h = run_pointwise(c1, [ops.Src(xin)], act=act)
        if carry_stats is None:
            carry_stats = isinstance(c2, Conv2d)
        if not carry_stats:
            return run_pointwise(c2, [ops.Src(h)], act=act)
        # the output carries its GroupNorm(1) moments (a U-Net processor's first norm reads it): no statistics pass
        st = ops.new_stats(h.shape[0], h)
        return ops.attach_stats(run_pointwise(c2, [ops.Src(h)], act=act, out_stats=st), st)

    def run_packed_ad(self, xin):
        """Differentiable form of run_packed (the packed input is data: no gradient flows into it)."""
        act = activation_code(self.encoder[1])
        h = ad.act(self.encoder[0].run_ad(xin), act)
        return ad.act(self.encoder[2].run_ad(h), act)

    def forward(self, u: torch.Tensor, pos: torch.Tensor, variables_broadcast: torch.Tensor = None, **kwargs):
        """u (B, c, tw, *spatial), pos (B, *spatial, nd) (1-D: also (B, L)), variables_broadcast (B, n_cond, *spatial)
        on a 1-D, 2-D or 3-D grid -> (B, hidden, *spatial)."""
        B, spatial = u.shape[0], tuple(u.shape[3:])
        vb = variables_broadcast
        Cp = ((self.n_in + 3) // 4) * 4
        # the broadcast conditioning is already a spatial field here: pass it as spatial channels
        xin, _ = ops.pack_grid_input(u.contiguous(), pos.float().contiguous(), None,
                                     vb.float().contiguous() if vb is not None else None, Cp)
        xin = xin.view((B,) + flat_frame(spatial) + (Cp,))
        if use_autograd(self):
            y = ad.to_nchw(self.run_packed_ad(xin))
        else:
            y = ops.nhwc_to_nchw(self.run_packed(xin))
        return y.view((B, y.shape[1]) + spatial)
