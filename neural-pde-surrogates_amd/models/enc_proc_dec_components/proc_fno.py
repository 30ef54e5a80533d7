"""FNO processor and spectral convolutions (reference models/enc_proc_dec_components/proc_fno.py).

Same classes, constructor kwargs and parameters (weights1/weights2 complex64
(Cin, Cout, m1, m2)) as the reference; forward runs the truncated-DFT HIP
pipeline (nps_hip.ops.spectral_conv2d; 1-D: ops.spectral_conv1d).  Internal
entry points `run(...)` take NHWC tensors / virtual frames so composite models
never transpose.
"""
from typing import Callable, NamedTuple

import torch
from torch import nn

from common.interfaces import D, M
from models.common import (get_conv_with_right_spatial_dim, activation_code, use_autograd, run_flat, run_pointwise,
                           AUTOGRAD2D, BF16FLAT)
from nps_hip import ops
from nps_hip import autograd as ad
from pdes import PDE


class FNO(nn.Module):
    """proc_fno.py:22-83."""
    model_interface = M.AR_TB
    data_interface = [D.sim1d, D.sim1d_var_t, D.sim2d]

    def __init__(self, pde: PDE, num_spatial_dims: int = 1, n_cond: int = 0, hidden_features: int = 128,
                 fno_modes: int = 48, hidden_blocks: int = 4, cond_mode: str = "concat", fno_kernel_size: int = 1,
                 fno_conv_mode: str = "single", padding_mode: str = "circular", **kwargs):
        super().__init__()
        self.pde = pde
        self.num_spatial_dims = num_spatial_dims
        self.cond_mode = cond_mode
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
            padding_mode=padding_mode if padding_mode != "ones" else "zeros",
        ) for _ in range(hidden_blocks)])

    def __repr__(self):
        return f'FNO{self.num_spatial_dims}D'

    def _film_p(self, variables):
        """The layers' FiLM operand: `variables` (B, n_cond) for cond_mode "film" with n_cond > 0, else None."""
        if self.cond_mode != "film" or not self.fno_layers[0].conv.feature_transform:
            return None  # film with n_cond == 0 is a plain FNO
        if self.num_spatial_dims not in (1, 2):
            raise NotImplementedError(SpectralConv3d.FILM_MSG if self.num_spatial_dims == 3 else
                                      "FiLM conditioning is on the MI355X path for 1-D and 2-D FNOs only")
        if variables is None:
            raise NotImplementedError(
                "FNO(cond_mode='film') needs `variables` (B, n_cond): call forward(h, variables=...).  The reference "
                "does not route `variables` to processors either (EncProcDec hands them variables_broadcast only), "
                "so FiLM is a module-level feature")
        return variables

    def _layers(self, h, vb, step):
        """The layer loop of run / run_ad / run_bf16: h = step(layer, srcs) on each layer's virtual input frame, (h | vb)
        for cond_mode "concat"."""
        for layer in self.fno_layers:
            srcs = [ops.Src(h)] + ([ops.Src(vb)] if (vb is not None and self.cond_mode == "concat") else [])
            h = step(layer, srcs)
        return h

    def run(self, h, vb, D=None, variables=None):
        """NHWC: h (B,H,W,C), vb (B,H,W,K) or None (3-D: NDHWC viewed as (B, D*H, W, C), depth D; 1-D: channels-last
        (B, L, C) viewed as (B, 1, L, C)); variables (B, n_cond): the FiLM operand of cond_mode "film"."""
        p = self._film_p(variables)
        return self._layers(h, vb, lambda layer, srcs: layer.run(srcs, D=D, p=p))

    def run_ad(self, h, vb, D=None, variables=None):
        p = self._film_p(variables)
        return self._layers(h, vb, lambda layer, srcs: layer.run_ad(ad.frame(srcs, srcs[0].t.shape[1:3]), D, p))

    def run_bf16(self, h, vb, D):
        """bf16-storage forward of a 3-D FNO (BASELINE config C5): h (B, D*H, W, C), vb (B, D*H, W, K) bf16
        NDHWC views; every layer in bf16 storage with fp32 arithmetic (FNO_Layer.run_bf16)."""
        if self.num_spatial_dims != 3:
            raise NotImplementedError("the bf16 storage path is the 3-D FNO's (config C5)")
        if self.cond_mode == "film":
            raise NotImplementedError("FiLM conditioning is not on the bf16 storage path")
        return self._layers(h, vb, lambda layer, srcs: layer.run_bf16(srcs, D))

    def forward(self, h: torch.Tensor, variables: torch.Tensor = None, variables_broadcast: torch.Tensor = None,
                pos=None):
        self._film_p(variables)  # a FiLM FNO without `variables`, or in 3-D, raises before any work
        rank = _RANKS[self.num_spatial_dims]
        for layer in self.fno_layers:
            rank.refuse_early(layer)  # (1-D: fno_kernel_size > 1)
        if rank.bf16 and h.dtype == torch.bfloat16 and use_autograd(self):
            raise NotImplementedError("the bf16 3-D FNO path is inference-only (fp32 for training)")

        def layers(form, h, vb, spatial):
            kw = {} if form is BF16FLAT else dict(variables=variables)
            return getattr(self, form.run)(h, vb, spatial[0] if rank.depth else None, **kw)
        return run_flat(self, h, variables_broadcast, layers, bf16=rank.bf16)


class FNO_Layer(nn.Module):
    """proc_fno.py:87-155: spectral conv + `w` conv (+ `w2`), then optional GELU — one fused output pass."""

    def __init__(self, hidden_dim, num_spatial_dims: int = 1, kernel_size=1, modes=16, activation=nn.GELU,
                 activation_params=None, feature_transform=False, feature_transform_dim=6, transform_mode=0,
                 hidden_dim_out=None, conv_mode="single", padding_mode="circular"):
        super().__init__()
        self.num_spatial_dims = num_spatial_dims
        assert conv_mode in ["single", "double"]
        self.conv_mode = conv_mode
        if isinstance(modes, int):
            modes = tuple([modes for _ in range(num_spatial_dims)])
        assert len(modes) == num_spatial_dims, 'modes should be int or tuple of ints with length equal to spatial dim!'
        self.modes = modes
        if hidden_dim_out is None:
            hidden_dim_out = hidden_dim
        self.conv = get_spectral_conv_with_right_spatial_dim(
            spatial_dim=num_spatial_dims, in_channels=hidden_dim, out_channels=hidden_dim_out, modes=modes,
            feature_transform=feature_transform, feature_transform_dim=feature_transform_dim,
            transform_mode=transform_mode)
        if conv_mode == "single":
            self.w = get_conv_with_right_spatial_dim(spatial_dim=num_spatial_dims, in_channels=hidden_dim,
                                                     out_channels=hidden_dim_out, kernel_size=kernel_size,
                                                     padding='same', padding_mode=padding_mode)
        else:
            self.w = get_conv_with_right_spatial_dim(spatial_dim=num_spatial_dims, in_channels=hidden_dim,
                                                     out_channels=hidden_dim_out, kernel_size=1, padding='same')
            self.w2 = get_conv_with_right_spatial_dim(spatial_dim=num_spatial_dims, in_channels=hidden_dim,
                                                      out_channels=hidden_dim_out, kernel_size=kernel_size,
                                                      padding='same', padding_mode=padding_mode)
        if activation is None:
            self.act = None
        else:
            self.act = activation(**(activation_params or {}))

    def _check_modes(self, spat_dim):
        for i, s in enumerate(spat_dim):  # proc_fno.py:134-139
            if i == len(spat_dim) - 1:
                assert self.modes[i] <= s // 2 + 1, \
                    'modes should be at most the spatial dim // 2 + 1 for the last spatial dimension!'
            else:
                assert self.modes[i] <= s, 'modes should be at most the spatial dim all but the last spatial dimensions!'

    def _check_1d(self):
        if any(tuple(c.kernel_size) != (1,) for c in (self.w, getattr(self, "w2", self.w))):
            raise NotImplementedError("FNO_Layer 1-D: fno_kernel_size > 1 is not on the MI355X path (pointwise `w` "
                                      "convs only)")

    def run(self, srcs, act_override=None, D=None, p=None):
        """srcs: virtual NHWC input frame (h, vb) — for 3-D layers NDHWC sources viewed as (B, D*H, W, C), depth D; for
        1-D layers (B, 1, L, C) views; p (B, K): the FiLM operand of a 1-D / 2-D layer with feature_transform.  Returns
        act(spectral(x) + w(x) [+ w2(x)])."""
        rank = _RANKS[self.num_spatial_dims]
        H, W = srcs[0].t.shape[1:3]
        self._check_modes(rank.spatial((H, W), D, "sources"))
        rank.refuse(self)
        act = activation_code(self.act) if act_override is None else act_override
        if (rank.fused and self.conv_mode != "double"
                and ops.spectral_fusable(W, self.conv.modes2, self.conv.out_channels)):
            # conv(x) + w(x) in one output pass: the 1x1's epilogue synthesises the spectral conv's W pass
            # (nps_conv2d_t.spec_z; scale 1 / (H W) of irfft2's norm), then the activation.  FiLM acts on the mixed
            # modes, before Z is formed, so a FiLM layer takes the same route
            Z = self.conv.run_z(srcs, p=p)
            return self.w.run(srcs, (H, W), spec=(Z, self.conv.modes2, 1.0 / (H * W)), act=act)
        out = run_pointwise(self.w, srcs)  # (a 1-D layer's pixels fold into 32-point rows)
        if self.conv_mode == "double":
            run_pointwise(self.w2, srcs, out=out, accumulate=True)
        return self.conv.run(srcs, out=out, accumulate=True, act=act, p=p, D=D)

    def run_bf16(self, srcs, D, act_override=None):
        """3-D layer in bf16 storage: act(spectral(x) + w(x)) with bf16 sources / output, fp32 sums."""
        if self.num_spatial_dims != 3 or self.conv_mode != "single":
            raise NotImplementedError("bf16 storage: 3-D FNO layers with conv_mode 'single' (config C5)")
        DH, W = srcs[0].t.shape[1:3]
        self._check_modes((D, DH // D, W))
        act = activation_code(self.act) if act_override is None else act_override
        out = self.w.run_bf16(srcs)
        return self.conv.run_bf16(srcs, D, out=out, accumulate=True, act=act)

    def run_ad(self, x, D=None, p=None):
        """Differentiable form: x (B,H,W,Cin) materialised frame ((B, D*H, W, Cin) for 3-D layers, (B, 1, L, Cin) for
        1-D ones); p as in run."""
        rank = _RANKS[self.num_spatial_dims]
        self._check_modes(rank.spatial(tuple(x.shape[1:3]), D, "tensors"))
        rank.refuse(self)
        y = ad.add_at(self.conv.run_ad(x, p=p, D=D), self.w.run_ad(x))
        if self.conv_mode == "double":
            y = ad.add_at(y, self.w2.run_ad(x))
        return ad.act(y, activation_code(self.act))

    def forward(self, x, p=None):
        rank = _RANKS[self.num_spatial_dims]
        rank.refuse_early(self)

        def layer(form, h, _, spatial):
            D = spatial[0] if rank.depth else None
            return self.run_ad(h, D, p) if form is AUTOGRAD2D else self.run([ops.Src(h)], D=D, p=p)
        return run_flat(self, x, None, layer)


def _line(hw, D, what):
    assert hw[0] == 1, f"1-D layers take channels-last (B, L, C) {what} viewed as (B, 1, L, C)"
    return hw[1:]


def _refuse_double(layer):
    if layer.conv_mode != "single":
        raise NotImplementedError("FNO_Layer 3-D: conv_mode 'single' only on the MI355X path")


def _refuse_film(layer):
    if layer.conv.feature_transform:
        raise NotImplementedError(SpectralConv3d.FILM_MSG)


class _Rank(NamedTuple):
    """What differs between the grid ranks in the one run / run_ad / forward body of an FNO layer."""
    spatial: Callable       # ((rows, row) of the flat frame, D, what the caller passed) -> the grid's sizes (_check_modes)
    refuse: Callable        # layer -> raises what run / run_ad refuse at this rank, after the modes check
    refuse_early: Callable  # layer -> raises what forward() refuses before its layout transposes
    depth: bool = False     # a depth D accompanies the (D*H, W) frame
    fused: bool = False     # the `w` conv can take the spectral conv's W pass (ops.spectral_fusable)
    bf16: bool = False      # the FNO has a bf16-storage form


_RANKS = {
    1: _Rank(_line, FNO_Layer._check_1d, FNO_Layer._check_1d),
    2: _Rank(lambda hw, D, what: hw, lambda layer: None, lambda layer: None, fused=True),
    3: _Rank(lambda hw, D, what: (D, hw[0] // D, hw[1]), _refuse_double, _refuse_film, depth=True, bf16=True),
}


def _film(conv, p):
    """ops' FiLM operand (p, weights_feat.weight, weights_feat.bias, transform_mode) of a SpectralConv1d / 2d; None
    without feature_transform (p is then ignored, as in the reference)."""
    if not conv.feature_transform:
        return None
    assert p is not None  # proc_fno.py:210, :272: we must have supplied params
    return (p, conv.weights_feat.weight, conv.weights_feat.bias, conv.transform_mode)


class SpectralConv2d(nn.Module):
    """proc_fno.py:225-288: rfft2 -> per-mode complex mixing of the 2 retained corners -> irfft2."""

    def __init__(self, in_channels, out_channels, modes: tuple, feature_transform=False, feature_transform_dim=6,
                 transform_mode=1):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.modes1 = modes[0]
        self.modes2 = modes[1]
        self.scale = (1 / (in_channels * out_channels))
        self.weights1 = nn.Parameter(
            self.scale * torch.rand(in_channels, out_channels, self.modes1, self.modes2, dtype=torch.cfloat))
        self.weights2 = nn.Parameter(
            self.scale * torch.rand(in_channels, out_channels, self.modes1, self.modes2, dtype=torch.cfloat))
        self.feature_transform = feature_transform
        self.feature_transform_dim = feature_transform_dim
        self.transform_mode = transform_mode
        if feature_transform:
            self.weights_feat = nn.Linear(feature_transform_dim, self.out_channels * 2 * self.modes1 * self.modes2)

    def packed(self, H):
        w1, w2 = self.weights1, self.weights2
        key = (H, w1.data_ptr(), w1._version, w2.data_ptr(), w2._version, str(w1.device))
        if getattr(self, "_pk_key", None) != key:
            self._pk = ops.pack_spectral_weight(w1, w2, H)
            self._pk_key = key
        return self._pk

    def run(self, srcs, out=None, accumulate=False, addend=None, act=0, p=None, D=None):
        """srcs: NHWC sources.  Returns (B, H, W, Cout), or `out`.  (D: the depth a 3-D layer passes; none here.)"""
        H = srcs[0].t.shape[1]
        return ops.spectral_conv2d(srcs, self.packed(H), self.modes1, self.modes2, self.out_channels, out=out,
                                   accumulate=accumulate, addend=addend, act=act, film=_film(self, p))

    def run_ad(self, x, p=None, D=None):
        """Differentiable form on an NHWC tensor."""
        return ad.spectral_conv2d_film(self, x, p) if self.feature_transform else ad.spectral_conv2d(self, x)

    def run_z(self, srcs, p=None):
        """The spectrum Z (B, H, m2, Cout) before the W-pass synthesis (ops.spectral_z): the FNO layer hands it to
        its 1x1 `w`, whose epilogue synthesises it (conv2d(spec=...))."""
        H = srcs[0].t.shape[1]
        return ops.spectral_z(srcs, self.packed(H), self.modes1, self.modes2, self.out_channels, film=_film(self, p))

    def forward(self, x, p=None):
        film = _film(self, p)
        # the module's own NCHW tensors go straight to the channels-first W passes: no layout round trip
        H, W = x.shape[2:4]
        if not (self.modes1 <= H and self.modes2 <= W // 2 + 1):
            raise AssertionError("modes should be at most the spatial dim (// 2 + 1 for the last spatial dimension)")
        if use_autograd(self):
            return ad.spectral_conv2d_nchw(self, x) if film is None else ad.spectral_conv2d_film_nchw(self, x, p)
        return ops.spectral_conv2d_nchw(x, self.packed(H), self.modes1, self.modes2, self.out_channels, film=film)


class SpectralConv1d(nn.Module):
    """proc_fno.py:158-222: rfft -> per-mode complex mixing of the first `modes1` bins (times the FiLM factor) ->
    irfft, on the L-split truncated-DFT HIP kernels (include/nps.h, SpectralConv1d)."""

    def __init__(self, in_channels, out_channels, modes: tuple, feature_transform=False, feature_transform_dim=6,
                 transform_mode=1):
        super().__init__()
        self.in_channels, self.out_channels, self.modes1 = in_channels, out_channels, modes[0]
        self.scale = (1 / (in_channels * out_channels))
        self.weights1 = nn.Parameter(self.scale * torch.rand(in_channels, out_channels, self.modes1,
                                                             dtype=torch.complex64))
        self.feature_transform = feature_transform
        self.feature_transform_dim = feature_transform_dim
        self.transform_mode = transform_mode
        if feature_transform:
            self.weights_feat = nn.Linear(feature_transform_dim, self.out_channels * self.modes1)

    def packed(self):
        w = self.weights1
        key = (w.data_ptr(), w._version, str(w.device))
        if getattr(self, "_pk_key", None) != key:
            self._pk = ops.pack_spectral1d_weight(w)
            self._pk_key = key
        return self._pk

    def run(self, srcs, out=None, accumulate=False, addend=None, act=0, p=None, D=None):
        """srcs: channels-last (B, L, C) sources, or their (B, 1, L, C) views.  Returns (B, L, Cout), or `out`."""
        return ops.spectral_conv1d(srcs, self.packed(), self.modes1, self.out_channels, out=out,
                                   accumulate=accumulate, addend=addend, act=act, film=_film(self, p))

    def run_ad(self, x, p=None, D=None):
        """Differentiable form on a channels-last (B, L, Cin) tensor (or its (B, 1, L, Cin) view)."""
        return ad.spectral_conv1d_film(self, x, p) if self.feature_transform else ad.spectral_conv1d(self, x)

    def forward(self, x, p=None):
        _film(self, p)  # feature_transform without p
        ops.check_modes1d(x.shape[2], self.modes1)
        # x (B, C, L) is transposed on its (B, C, 1, L) view; the inference form hands back (B, L, Cout)
        return run_flat(self, x, None, lambda form, h, _, spatial: (
            self.run_ad(h, p) if form is AUTOGRAD2D else self.run([ops.Src(h)], p=p).unsqueeze(1)))


class SpectralConv3d(nn.Module):
    """proc_fno.py:291-376: rfftn over (D, H, W) -> per-mode complex mixing of the 4 retained corners ->
    irfftn, on the per-axis truncated-DFT HIP pipeline (include/nps.h, SpectralConv3d)."""
    FILM_MSG = ("SpectralConv3d FiLM is not built: the reference's own branch (proc_fno.py:351-370) cannot run (its "
                "shapes mismatch unless modes3 == W // 2 + 1, and it writes the same slice four times)")

    def __init__(self, in_channels, out_channels, modes: tuple, feature_transform=False, feature_transform_dim=6,
                 transform_mode=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.modes1, self.modes2, self.modes3 = modes[0], modes[1], modes[2]
        self.scale = (1 / (in_channels * out_channels))
        for i in range(1, 5):
            setattr(self, f"weights{i}", nn.Parameter(self.scale * torch.rand(
                in_channels, out_channels, self.modes1, self.modes2, self.modes3, dtype=torch.cfloat)))
        self.feature_transform = feature_transform
        self.feature_transform_dim = feature_transform_dim
        self.transform_mode = transform_mode
        if feature_transform:
            self.weights_feat = nn.Linear(feature_transform_dim,
                                          self.out_channels * 2 * self.modes1 * 2 * self.modes2 * self.modes3)

    def _weights(self):
        return [self.weights1, self.weights2, self.weights3, self.weights4]

    def packed(self, D, H):
        ws = self._weights()
        key = (D, H, str(ws[0].device)) + tuple((w.data_ptr(), w._version) for w in ws)
        if getattr(self, "_pk_key", None) != key:
            self._pk = ops.pack_spectral3d_weight(ws, D, H)
            self._pk_key = key
        return self._pk

    def packed_bf16(self, D, H):
        wp = self.packed(D, H)
        if getattr(self, "_pkb_src", None) is not wp:
            self._pkb = ops.to_bf16(wp)
            self._pkb_src = wp
        return self._pkb

    def run_bf16(self, srcs, D, out=None, accumulate=False, addend=None, act=0):
        """bf16-storage form: bf16 NDHWC sources viewed as (B, D*H, W, C) -> bf16 (B, D*H, W, Cout)."""
        if self.feature_transform:
            raise NotImplementedError(self.FILM_MSG)
        H = srcs[0].t.shape[1] // D
        return ops.spectral_conv3d_bf16(srcs, D, self.packed_bf16(D, H), self.modes1, self.modes2, self.modes3,
                                        self.out_channels, out=out, accumulate=accumulate, addend=addend, act=act)

    def run(self, srcs, D=None, out=None, accumulate=False, addend=None, act=0, p=None):
        """srcs: NDHWC sources viewed as (B, D*H, W, C), depth D.  Returns (B, D*H, W, Cout).  (p: the FiLM operand
        a layer passes; FiLM is refused here.)"""
        if self.feature_transform:
            raise NotImplementedError(self.FILM_MSG)
        H = srcs[0].t.shape[1] // D
        return ops.spectral_conv3d(srcs, D, self.packed(D, H), self.modes1, self.modes2, self.modes3,
                                   self.out_channels, out=out, accumulate=accumulate, addend=addend, act=act)

    def run_ad(self, x, p=None, D=None):
        """Differentiable form on the (B, D*H, W, Cin) view of an NDHWC tensor, depth D."""
        return ad.spectral_conv3d(self, x, D)

    def forward(self, x, p=None):
        if self.feature_transform:
            raise NotImplementedError(self.FILM_MSG)
        B, C, D, H, W = x.shape
        ops.check_modes3d(D, H, W, self.modes1, self.modes2, self.modes3)
        if x.dtype == torch.bfloat16:  # bf16 storage (C5), inference only
            return run_flat(self, x, None, lambda form, h, _, spatial: self.run_bf16([ops.Src(h)], D), bf16=True)
        # fp32: the module's own NCDHW tensors go straight to the channels-first W passes
        if use_autograd(self):
            return ad.spectral_conv3d_nchw(self, x)
        return ops.spectral_conv3d_nchw(x, self.packed(D, H), self.modes1, self.modes2, self.modes3,
                                        self.out_channels)


def get_spectral_conv_with_right_spatial_dim(spatial_dim, **kwargs):
    """proc_fno.py:379-389."""
    if spatial_dim == 1:
        return SpectralConv1d(**kwargs)
    if spatial_dim == 2:
        return SpectralConv2d(**kwargs)
    if spatial_dim == 3:
        return SpectralConv3d(**kwargs)
    raise NotImplementedError(f'only 0<x<=3d convs implemented so far, but found spatial dim {spatial_dim}!')
