"""U-FNO processor (reference models/enc_proc_dec_components/proc_ufno.py).

Per block h = GELU(FNO_Layer(cat(h, vb)) + UNetModern(h, vb)): the FNO branch
(1x1 conv + truncated-DFT spectral conv accumulated in one output pass) is
written once, and the U-Net's final conv epilogue adds it and applies GELU,
so the block output is produced by that single launch.
"""
from typing import List, Tuple, Union

import torch
from torch import nn

from common.interfaces import D, M
from models.common import activation_code, use_autograd, run_flat, to_ndhwc, to_ncdhw, ad_to_ndhwc, ad_to_ncdhw
from models.enc_proc_dec_components.proc_fno import FNO_Layer
from models.enc_proc_dec_components.proc_unet_modern import UNetModern
from nps_hip import ops
from nps_hip import autograd as ad
from pdes import PDE


class UFNO(nn.Module):
    """proc_ufno.py:25-118."""
    model_interface = M.AR_TB
    data_interface = [D.sim1d, D.sim1d_var_t, D.sim2d]

    def __init__(self, pde: PDE, num_spatial_dims: int = 1, n_cond: int = 0, hidden_features: int = 128,
                 hidden_blocks: int = 4, cond_mode: str = "concat", padding_mode: str = "circular",
                 fno_modes: int = 48, fno_kernel_size: int = 1, fno_conv_mode: str = "single",
                 activation: nn.Module = nn.GELU(), norm: bool = False,
                 ch_mults: Union[Tuple[int, ...], List[int]] = (1, 1, 1),
                 is_attn: Union[Tuple[bool, ...], List[bool]] = (False, False, False), mid_attn: bool = False,
                 n_blocks: int = 1, use1x1: bool = True, **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.cond_mode = cond_mode
        self.activation = activation
        assert self.cond_mode in ["film", "concat", None], "Incorrect conditioning mode supplied"
        if self.cond_mode == "film":
            feature_transform, feature_transform_dim, hidden_dim_in = n_cond > 0, n_cond, hidden_features
        elif self.cond_mode == "concat":
            feature_transform, feature_transform_dim, hidden_dim_in = False, 0, hidden_features + n_cond
        else:
            feature_transform, feature_transform_dim, hidden_dim_in = False, 0, hidden_features
        self.fno_layers = nn.ModuleList([FNO_Layer(
            hidden_dim=hidden_dim_in, hidden_dim_out=hidden_features, num_spatial_dims=num_spatial_dims,
            modes=fno_modes, feature_transform=feature_transform, feature_transform_dim=feature_transform_dim,
            kernel_size=fno_kernel_size, conv_mode=fno_conv_mode,
            padding_mode=padding_mode if padding_mode != "ones" else "zeros", activation=None,
        ) for _ in range(hidden_blocks)])
        self.unet_layers = nn.ModuleList([UNetModern(
            pde=pde, num_spatial_dims=num_spatial_dims, n_cond=n_cond, hidden_features=hidden_features,
            cond_mode=cond_mode, activation=activation, norm=norm, ch_mults=ch_mults, is_attn=is_attn,
            mid_attn=mid_attn, n_blocks=n_blocks, use1x1=use1x1, padding_mode=padding_mode,
        ) for _ in range(hidden_blocks)])

    def __repr__(self):
        return f'U-FNO{self.num_spatial_dims}D'

    def _check_concat(self):
        if self.cond_mode != "concat":
            raise NotImplementedError("U-FNO: only cond_mode='concat' runs on the MI355X path")

    def _blocks(self, h, vb, view, fno_run, fork, unet_run, unview):
        """The inference block loop.  view: h / vb as the FNO layer's (B, rows, row, C) sources; fno_run(fno, srcs) the
        layer's output; fork(h, settle) the ops.Fork it runs in; unet_run the U-Net method, whose final conv adds the
        layer's output, seen through unview as a map like h, and applies the activation."""
        act = activation_code(self.activation)
        for fno, unet in zip(self.fno_layers, self.unet_layers):
            srcs = [ops.Src(view(h))] + ([ops.Src(view(vb))] if vb is not None else [])
            # the FNO layer and the U-Net read the same h: the FNO layer runs on a side stream (ops.Fork,
            # lane 1) beside the U-Net, whose final conv joins it and adds its output
            f = fork(h, [s.t for s in srcs])
            with f:
                h_fno = fno_run(fno, srcs)
            h = getattr(unet, unet_run)(h, vb, addend=unview(h_fno), act_after=act, addend_fork=f)
        return h

    def _blocks_ad(self, h, vb, view, D, unet_run, unview):
        """The autograd block loop: per block the FNO layer on the frame of (h, vb) seen through view (depth D) plus
        the U-Net's output seen through view, then the activation, seen through unview as a map like h."""
        act = activation_code(self.activation)
        for fno, unet in zip(self.fno_layers, self.unet_layers):
            srcs = [ops.Src(view(h))] + ([ops.Src(view(vb))] if vb is not None else [])
            h_fno = fno.run_ad(ad.frame(srcs, srcs[0].t.shape[1:3]), D)
            h = unview(ad.act(ad.add_at(h_fno, view(getattr(unet, unet_run)(h, vb))), act))
        return h

    def run(self, h, vb):
        """NHWC (1-D: the (B, 1, L, C) maps).  The fork is on for small activations (ops.fno_fork)."""
        self._check_concat()
        same = lambda t: t  # noqa: E731
        return self._blocks(h, vb, same, lambda fno, srcs: fno.run(srcs),
                            lambda h, settle: ops.fno_fork(h, settle=settle), "run", same)

    def run3d(self, h, vb):
        """3-D U-FNO (BASELINE config C5) on NDHWC (B, D, H, W, C) activations, fp32 or bf16 storage: per
        block the FNO-3D layer on cat(h, vb) (the (B, D*H, W, C) view), then the 3-D U-Net whose final conv
        epilogue adds it and applies the activation (proc_ufno.py:105-118).  The FNO layer forks at every size (C5 at
        B = 8 +1 %, profiles/r4/experiments/side_stream_forks_ab.txt)."""
        self._check_concat()
        if self.num_spatial_dims != 3:
            raise NotImplementedError("UFNO.run3d: 3-D only")
        B, D, H, W = h.shape[:4]
        fno_run = ((lambda fno, srcs: fno.run_bf16(srcs, D)) if h.dtype == torch.bfloat16 else
                   (lambda fno, srcs: fno.run(srcs, D=D)))
        return self._blocks(h, vb, lambda t: t.view(t.shape[0], D * H, W, t.shape[4]), fno_run,
                            lambda h, settle: ops.Fork(h, lane=1, on=ops.SIDE_FNO, settle=settle), "run3d",
                            lambda t: t.view(B, D, H, W, t.shape[3]))

    def run_ad(self, h, vb):
        """Differentiable form of run() (training)."""
        self._check_concat()
        same = lambda t: t  # noqa: E731
        return self._blocks_ad(h, vb, same, None, "run_ad", same)

    def run_ad3d(self, h, vb):
        """Differentiable form of run3d() on NDHWC fp32 (training): (h, vb) carry no offsets, so the FNO-3D layer's
        frame is the 2-D frame of the (B, D*H, W, C) view."""
        self._check_concat()
        if self.num_spatial_dims != 3:
            raise NotImplementedError("UFNO.run_ad3d: 3-D only")
        B, D, H, W = h.shape[:4]
        return self._blocks_ad(h, vb, lambda t: t.view(t.shape[0], D * H, W, t.shape[4]), D, "run_ad3d",
                               lambda t: t.view(B, D, H, W, -1))

    def forward(self, h: torch.Tensor, variables: torch.Tensor = None, variables_broadcast: torch.Tensor = None,
                pos=None):
        if self.num_spatial_dims == 3:  # the U-Nets walk NDHWC volumes: the one boundary that is not the flat frame's
            return self._forward3d(h, variables_broadcast)
        if self.num_spatial_dims == 1:
            for unet in self.unet_layers:
                unet.check_1d()  # a circular 1-D U-Net raises before any work
            for layer in self.fno_layers:
                layer._check_1d()  # fno_kernel_size > 1
        return run_flat(self, h, variables_broadcast, lambda form, h, vb, spatial: getattr(self, form.run)(h, vb))

    def _forward3d(self, h, vb):
        """(B, C, D, H, W), fp32 or bf16 storage (C5)."""
        if use_autograd(self):
            if h.dtype != torch.float32 or (vb is not None and vb.dtype != torch.float32):
                raise NotImplementedError("the 3-D U-FNO differentiates fp32 tensors only: use fp32 for training "
                                          "(bf16 storage is the inference path)")
            return ad_to_ncdhw(self.run_ad3d(ad_to_ndhwc(h), ad_to_ndhwc(vb) if vb is not None else None))
        vb = to_ndhwc(vb) if vb is not None else None
        if vb is not None and vb.dtype != h.dtype:  # conditioning in the activations' storage dtype
            vb = ops.to_bf16(vb) if h.dtype == torch.bfloat16 else ops.to_f32(vb)
        return to_ncdhw(self.run3d(to_ndhwc(h), vb))
