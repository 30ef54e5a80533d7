"""Conv building blocks of the grid models (reference models/common.py).

The parameter-holding classes subclass torch.nn's Conv2d / ConvTranspose2d /
GroupNorm so construction, initialisation and `state_dict` keys are identical
to the reference; their forward never calls aten convolution: it runs the
gfx950 implicit-GEMM kernel through nps_hip (fails loudly off-GPU).
"""
import copy
from typing import Callable, NamedTuple

import torch
from torch import nn

from nps_hip import ops
from nps_hip import autograd as ad


def use_autograd(module) -> bool:
    """True when this forward must be differentiable (training): grad mode on and trainable parameters.
    The differentiable path runs the same HIP kernels unfused plus their backward kernels (nps_hip.autograd)."""
    return torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


class Swish(nn.Module):
    """common.py:7-17: x * sigmoid(beta x).  The one place the models use it, dec_grid.TimeConv's chain, applies it
    inside the decode kernel (NPS_DECODE_ACT_SWISH with this beta); forward is the same function in torch ops, on
    whatever tensor it is given."""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta

    def forward(self, x):
        return x * torch.sigmoid(self.beta * x)


def activation_code(act):
    """Map an activation module to the fused-epilogue code of the HIP kernels."""
    if act is None or isinstance(act, nn.Identity):
        return 0
    if isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none":
        return ops.GELU
    raise NotImplementedError(f"activation {act!r} is not fused on the MI355X path (GELU only)")


def crop_offsets(cur, des):
    """Per-axis placement of a cur-sized map / volume inside a des-sized frame, crop_Nd semantics (common.py:20-34)."""
    return tuple(ops.crop_offset(c, d) for c, d in zip(cur, des))


def crop_Nd(num_spatial_dims, enc_ftrs, shape):
    """common.py:20-34 on NCHW device tensors (module-boundary helper; the fused paths never call it)."""
    if num_spatial_dims != 2:
        raise NotImplementedError("crop_Nd: 2-D only on the MI355X path")
    if isinstance(shape, torch.Tensor):
        shape = shape.shape
    H, W = shape[-2], shape[-1]
    B, C, h, w = enc_ftrs.shape
    oy, ox = crop_offsets((h, w), (H, W))
    x = ops.nchw_to_nhwc(enc_ftrs)
    out = torch.zeros((B, H, W, C), dtype=torch.float32, device=x.device)
    y0, y1 = max(0, oy), min(H, oy + h)
    x0, x1 = max(0, ox), min(W, ox + w)
    out[:, y0:y1, x0:x1] = x[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return ops.nhwc_to_nchw(out)


class _PackedMixin:
    """Caches the MFMA-packed copy of `weight`, re-packed when the parameter changes."""

    def _packed(self, fn, kind="conv"):
        return ops.cached_pack(self.weight, kind, fn)


class Conv2d(_PackedMixin, nn.Conv2d):
    """nn.Conv2d parameters; forward = fused HIP implicit-GEMM conv (NHWC internally)."""

    def geometry(self):
        """(KH, KW, stride, dil, pad_top_left, pad_bottom_right, circ) of this conv."""
        KH, KW = self.kernel_size
        if self.stride[0] != self.stride[1] or self.dilation[0] != self.dilation[1]:
            raise NotImplementedError("anisotropic stride/dilation")
        s, d = self.stride[0], self.dilation[0]
        if self.padding == "same":
            tot = (d * (KH - 1), d * (KW - 1))
            lo = (tot[0] // 2, tot[1] // 2)
            hi = (tot[0] - lo[0], tot[1] - lo[1])
        elif self.padding == "valid":
            lo = hi = (0, 0)
        else:
            lo = hi = tuple(self.padding)
        if self.padding_mode == "circular":
            if lo != hi or lo[0] != lo[1]:
                raise NotImplementedError("asymmetric circular padding")
            return KH, KW, s, d, (0, 0), (0, 0), lo[0]
        if self.padding_mode != "zeros":
            raise NotImplementedError(f"padding_mode {self.padding_mode}")
        return KH, KW, s, d, lo, hi, 0

    def out_hw(self, H, W):
        """Output size of this conv on an (H, W) frame."""
        KH, KW, s, d, lo, hi, circ = self.geometry()
        return ((H + 2 * circ + lo[0] + hi[0] - d * (KH - 1) - 1) // s + 1,
                (W + 2 * circ + lo[1] + hi[1] - d * (KW - 1) - 1) // s + 1)

    def run(self, srcs, frame_hw, **kw):
        KH, KW, s, d, lo, hi, circ = self.geometry()
        x = srcs[0].t
        if (s == 2 and KH == 3 and KW == 3 and d == 1 and circ == 0 and lo == hi and lo[0] == lo[1]
                and len(srcs) == 1 and srcs[0].off_y == 0 and srcs[0].off_x == 0
                and tuple(x.shape[1:3]) == tuple(frame_hw) and x.shape[3] % 4 == 0
                and "gn" not in kw and not kw.get("pre_act")):
            # U-Net Downsample: 3x3/s2 as a 2x2 stride-1 conv over the space-to-depth input
            p = lo[0]
            Ho, Wo = self.out_hw(*frame_hw)
            pk2 = self._packed(ops.pack_conv_weight_s2d, "s2d")
            if ops.S2D_VIEW and x.shape[3] % 16 == 0 and pk2.nps_precision == ops.PREC_X3F16:
                # the split-fp16 producers read the space-to-depth view straight from x (nps_conv2d_t.s2d)
                return ops.conv2d([ops.Src(x)], (Ho + 1, Wo + 1), pk2, self.bias, self.out_channels, 2, 2,
                                  out_hw=(Ho, Wo), s2d_pad=p, **kw)
            xq = ops.space_to_depth(x, p, Ho + 1, Wo + 1)
            return ops.conv2d([ops.Src(xq)], (Ho + 1, Wo + 1), pk2, self.bias, self.out_channels, 2, 2,
                              out_hw=(Ho, Wo), **kw)
        pk = self._packed(lambda w: ops.pack_conv_weight(w, s, d), ("conv", s, d))
        return ops.conv2d(srcs, frame_hw, pk, self.bias, self.out_channels, KH, KW,
                          stride=s, dil=d, pad=lo, pad_bottom=hi, circ=circ, **kw)

    def run_ad(self, x):
        """Differentiable form on an NHWC tensor (the method Conv1d / Conv3d give their pointwise views)."""
        return ad.conv2d(self, x)

    def forward(self, x):
        if use_autograd(self):
            return ad.to_nchw(ad.conv2d(self, ad.to_nhwc(x)))
        x = ops.nchw_to_nhwc(x)
        y = self.run([ops.Src(x)], x.shape[1:3])
        return ops.nhwc_to_nchw(y)


class ConvTranspose2d(_PackedMixin, nn.ConvTranspose2d):
    """nn.ConvTranspose2d(k=4, s=2) parameters; forward = 4 phase convs on the HIP conv kernel.

    Output phase (py, px) of a stride-2 4x4 transposed conv is a 2x2 conv of the
    input with taps (py + 2(1-ty), px + 2(1-tx)), written to rows 2*qy+py."""
    pre_pad = 0  # circular pre-padding (ConvTranspose2d_padded)

    def run(self, x, act=0):
        if tuple(self.kernel_size) != (4, 4) or tuple(self.stride) != (2, 2) or tuple(self.dilation) != (1, 1) \
                or tuple(self.output_padding) != (0, 0) or self.groups != 1:
            raise NotImplementedError("only the U-Net Upsample transposed conv (k=4, s=2) runs on the MI355X path")
        p = self.padding[0]
        if self.padding[1] != p or p not in (0, 1):
            raise NotImplementedError("transposed conv padding must be 0 or 1")
        B, H, W, C = x.shape
        c = self.pre_pad
        Hp, Wp = H + 2 * c, W + 2 * c
        Ho, Wo = 2 * Hp + 2 - 2 * p, 2 * Wp + 2 - 2 * p
        out = ops.empty_nhwc(B, Ho, Wo, self.out_channels, x)
        phases = self._packed(ops.pack_convT_phases, "convT")
        st = ops.new_stats(B, x)  # the 4 phases store every output element once: GroupNorm(1) moments of out
        if getattr(phases[0], "nps_precision", None) == ops.PREC_X3F16 and ops.MERGE_CONVT_PHASES:
            # one launch: the phases' work-groups share each input patch (nps_conv2d_t.nphase)
            ops.conv2d([ops.Src(x)], (H, W), phases[0], self.bias, self.out_channels, 2, 2, pad=(1, 1), circ=c,
                       out_hw=(Hp + 1, Wp + 1), out=out, out_os=2, out_off=(-p, -p), act=act, out_stats=st, phases=4)
            return ops.attach_stats(out, st)
        for ph in range(4):
            py, px = ph >> 1, ph & 1
            ops.conv2d([ops.Src(x)], (H, W), phases[ph], self.bias, self.out_channels, 2, 2, pad=(1, 1), circ=c,
                       out_hw=(Hp + 1, Wp + 1), out=out, out_os=2, out_off=(py - p, px - p), act=act, out_stats=st)
        return ops.attach_stats(out, st)

    def forward(self, x):
        if use_autograd(self):
            return ad.to_nchw(ad.conv_transpose2d(self, ad.to_nhwc(x)))
        return ops.nhwc_to_nchw(self.run(ops.nchw_to_nhwc(x)))


class ConvTranspose2d_padded(ConvTranspose2d):
    """common.py:93-100: circular_pad_2d(x, pad) then the transposed conv (fused as circular frame extension)."""

    def __init__(self, pad, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pad = pad
        self.pre_pad = pad


def to_ndhwc(x):
    """(B, C, D, H, W) -> contiguous (B, D, H, W, C) on the HIP transpose (fp32; bf16 via fp32)."""
    B, C, D, H, W = x.shape
    bf = x.dtype == torch.bfloat16
    x4 = x.reshape(B, C, D * H, W)
    y = ops.nchw_to_nhwc(ops.to_f32(x4.contiguous()) if bf else x4)
    return (ops.to_bf16(y) if bf else y).view(B, D, H, W, C)


def to_ncdhw(y):
    """(B, D, H, W, C) -> (B, C, D, H, W) on the HIP transpose."""
    B, D, H, W, C = y.shape
    bf = y.dtype == torch.bfloat16
    y4 = y.reshape(B, D * H, W, C)
    x = ops.nhwc_to_nchw(ops.to_f32(y4) if bf else y4)
    return (ops.to_bf16(x) if bf else x).view(B, C, D, H, W)


def ad_to_ndhwc(x):
    """to_ndhwc of an fp32 tensor, differentiably: NCDHW -> NDHWC is the NCHW -> NHWC permutation of the
    (B, C, D*H, W) view."""
    B, C, D, H, W = x.shape
    return ad.to_nhwc(x.reshape(B, C, D * H, W)).view(B, D, H, W, C)


def ad_to_ncdhw(y):
    """to_ncdhw of an fp32 tensor, differentiably."""
    B, D, H, W, C = y.shape
    return ad.to_nchw(y.reshape(B, D * H, W, C)).view(B, C, D, H, W)


def _ad_ncdhw(fn, conv, x):
    """fn(conv, x) — ad.conv3d / ad.conv_transpose3d, on NDHWC — around the differentiable layout transposes of an
    fp32 (B, C, D, H, W) tensor."""
    return ad_to_ncdhw(fn(conv, ad_to_ndhwc(x)))


class _Packed3Mixin:
    """Caches the nps_conv3d packing of `weight` per storage dtype, re-packed when the parameter changes."""

    def _packed3(self, bf16: bool, transposed: bool = False):
        w = self.weight
        key = (w.data_ptr(), w._version, str(w.device), bf16)
        cache = self.__dict__.setdefault("_pk3", {})
        if cache.get("key_" + str(bf16)) != key:
            cache[bf16] = ops.pack_conv3d_weight(w, transposed=transposed, bf16=bf16)
            cache["key_" + str(bf16)] = key
        return cache[bf16]


class Conv3d(_Packed3Mixin, _PackedMixin, nn.Conv3d):
    """nn.Conv3d parameters (common.py:37-47 with spatial_dim 3).  The FNO-3D pointwise `w` conv
    (fno_kernel_size 1) runs as a 1x1 conv over the (D*H, W) view of NDHWC activations on the 2-D HIP
    conv kernels (run / run_bf16); the 3-D U-Net's convs (k = 1 or 3, stride 1 or 2, valid / zero / circular
    padding) run on the NDHWC implicit-GEMM kernel nps_conv3d (run3d)."""

    def geometry3d(self):
        """(K, stride, circ, zpad) of a cubic, isotropic, undilated conv."""
        ks, st, dl = set(self.kernel_size), set(self.stride), set(self.dilation)
        if len(ks) != 1 or len(st) != 1 or dl != {1} or self.groups != 1:
            raise NotImplementedError("3-D convs: cubic kernel, isotropic stride, no dilation or groups")
        K, s = ks.pop(), st.pop()
        if self.padding == "same":
            if K % 2 == 0:
                raise NotImplementedError("3-D 'same' padding with an even kernel")
            p = (K - 1) // 2
        elif self.padding == "valid":
            p = 0
        else:
            pads = set(self.padding)
            if len(pads) != 1:
                raise NotImplementedError("anisotropic 3-D padding")
            p = pads.pop()
        if self.padding_mode == "circular":
            return K, s, p, 0
        if self.padding_mode != "zeros":
            raise NotImplementedError(f"padding_mode {self.padding_mode}")
        return K, s, 0, p

    def out_dhw(self, dhw):
        """Output size of this conv on a (D, H, W) frame."""
        K, s, circ, zpad = self.geometry3d()
        return tuple((n + 2 * (circ + zpad) - K) // s + 1 for n in dhw)

    def run3d(self, srcs, frame_dhw, **kw):
        """srcs: ops.Src3 NDHWC sources (fp32 or bf16) of a virtual frame -> (B, Do, Ho, Wo, Cout)."""
        K, s, circ, zpad = self.geometry3d()
        bf16 = srcs[0].t.dtype == torch.bfloat16
        return ops.conv3d(srcs, frame_dhw, self._packed3(bf16), self.bias, self.out_channels, K, stride=s, circ=circ,
                          zpad=zpad, **kw)

    def _check(self):
        if tuple(self.kernel_size) != (1, 1, 1) or tuple(self.stride) != (1, 1, 1) or self.groups != 1 \
                or tuple(self.dilation) != (1, 1, 1):
            raise NotImplementedError("only pointwise (kernel 1) 3-D convs run on the MI355X path")

    def geometry(self):
        return 1, 1, 1, 1, (0, 0), (0, 0), 0

    def run(self, srcs, frame_hw, **kw):
        """srcs: NDHWC sources viewed as (B, D*H, W, C); frame_hw = (D*H, W)."""
        self._check()
        pk = self._packed(lambda w: ops.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1)), "conv1d")
        return ops.conv2d(srcs, frame_hw, pk, self.bias, self.out_channels, 1, 1, **kw)

    def run_bf16(self, srcs, act=0, addend=None):
        """bf16-storage form (C5): bf16 NDHWC sources viewed as (B, D*H, W, C) -> bf16 (B, D*H, W, Cout)."""
        self._check()
        w = self.weight
        key = ("bf16", w.data_ptr(), w._version, str(w.device))
        if getattr(self, "_pkb_key", None) != key:
            self._pkb = ops.pack_1x1_bf16(w)
            self._pkb_key = key
        return ops.conv1x1_bf16(srcs, self._pkb, self.bias, self.out_channels, act=act, addend=addend)

    def run_ad(self, x):
        self._check()
        return ad.Conv2dFn.apply(self.geometry(), x, self.weight.reshape(self.out_channels, self.in_channels, 1, 1),
                                 self.bias)

    def forward(self, x):
        if tuple(self.kernel_size) != (1, 1, 1) or tuple(self.stride) != (1, 1, 1):
            if use_autograd(self) and x.dtype == torch.float32:
                return _ad_ncdhw(ad.conv3d, self, x)
            return run_form(self, x, None, lambda form, x, _: self.run3d([form.Src(x)], x.shape[1:4]))
        return run_flat(self, x, None, lambda form, h, _, spatial: (
            self.run_ad(h) if form is AUTOGRAD2D else self.run([ops.Src(h)], h.shape[1:3])))


class Conv1d(_PackedMixin, nn.Conv1d):
    """nn.Conv1d parameters (common.py:37-47 with spatial_dim 1).  The FNO-1D pointwise `w` conv (fno_kernel_size 1)
    runs as a 1x1 conv over the (B, 1, L, C) view of channels-last activations on the 2-D HIP conv kernels; the 1-D
    U-Net's zero-padded k-tap convs (K <= 4, stride 1 or 2) run on the Conv1d kernels that tile along L
    (nps_conv1d_fwd), in fp32 (run / run_ad).  forward() of every non-pointwise geometry stays nn.Conv1d's own."""

    # set by the 1-D U-Net on its own pointwise convs (shortcuts, the final 1x1): they run on the exact-fp32 Conv1d
    # kernels with K = 1 like the k-tap convs around them, so that the U-Net's gradients carry fp32 rounding only (the
    # 2-D route's split-fp16 input gradients cost the parameter gradients behind them up to 1.7e-5); the FNO's `w`
    # keeps the 2-D route
    exact = False

    def pointwise(self):
        return (tuple(self.kernel_size) == (1,) and tuple(self.stride) == (1,) and tuple(self.dilation) == (1,)
                and self.groups == 1)

    def _taps(self):
        """True when run / run_ad take the Conv1d kernels (nps_conv1d_fwd)."""
        return self.padding_mode == "zeros" and (self.exact or not self.pointwise())

    def _check(self):
        if not self.pointwise():
            raise NotImplementedError("only pointwise (kernel 1) 1-D convs run on the MI355X path")

    def geometry1d(self):
        """(K, stride, pad_left, pad_right) of a zero-padded k-tap conv; every other geometry is refused (the message
        names the pointwise route, the one a circular conv could take with kernel 1)."""
        K, s = self.kernel_size[0], self.stride[0]
        if self.padding_mode != "zeros" or tuple(self.dilation) != (1,) or self.groups != 1 or K > 4 or s > 2:
            raise NotImplementedError(
                "1-D convs on the MI355X path: pointwise (kernel 1), or zero-padded with K <= 4, stride 1 or 2, no "
                f"dilation or groups; got kernel {K}, stride {s}, dilation {self.dilation[0]}, groups {self.groups}, "
                f"padding_mode {self.padding_mode!r}")
        if self.padding == "same":
            return K, s, (K - 1) // 2, K - 1 - (K - 1) // 2
        if self.padding == "valid":
            return K, s, 0, 0
        if s == 1 and self.padding[0] > K - 1:  # (the stride-1 input gradient pads dy by K - 1 - padding)
            raise NotImplementedError(f"1-D convs on the MI355X path: stride-1 padding {self.padding[0]} exceeds "
                                      f"kernel {K} - 1 (pointwise convs take no padding)")
        return K, s, self.padding[0], self.padding[0]

    def geometry(self):
        if self.pointwise():
            return 1, 1, 1, 1, (0, 0), (0, 0), 0
        K, s, pl, pr = self.geometry1d()
        return 1, K, s, 1, (0, pl), (0, pr), 0

    def out_hw(self, H, W):
        """Output size of this conv on a (1, L) frame."""
        if self.pointwise():
            return H, W
        K, s, pl, pr = self.geometry1d()
        return H, (W + pl + pr - K) // s + 1

    def _run_taps(self, srcs, frame_hw, gn=None, pre_act=0, out=None, out_off=(0, 0), accumulate=False, addends=(),
                  act=0, out_stats=None):
        """The k-tap route of run(): ops.conv2d's keywords on nps_conv1d_fwd.  A GroupNorm / activation prologue is
        materialised first (ops.frame_pack); the launch produces no GroupNorm moments (out_stats is marked
        incomplete: the next norm takes its statistics pass)."""
        K, s, pl, pr = self.geometry1d()
        if frame_hw[0] != 1 or len(addends) > 1:
            raise NotImplementedError("1-D convs take (1, L) frames and at most one addend")
        if gn is not None or pre_act:
            srcs = [ops.Src(ops.frame_pack(srcs, frame_hw, gn, pre_act))]
        if out_stats is not None:
            out_stats._nps_incomplete = True
        out3 = ad3 = None
        if out is not None:
            if out_off[0] != 0 or out.dim() != 4 or out.shape[1] != 1:
                raise RuntimeError("1-D conv: out must be a (B, 1, L, C) map written at row 0")
            ops.drop_stats(out)
            ops.drop_tag(out)
            out3 = out.view(out.shape[0], out.shape[2], out.shape[3])
        if len(addends) == 1:
            ad3 = addends[0].view(addends[0].shape[0], addends[0].shape[2], addends[0].shape[3])
        y = ops.conv1d(srcs, frame_hw[1], self._packed(ops.pack_conv1d_weight, "conv1"), self.bias, self.out_channels,
                       K, stride=s, pad=(pl, pr), out=out3, out_off=out_off[1], accumulate=accumulate, addend=ad3,
                       act=act)
        return out if out is not None else y.view(y.shape[0], 1, y.shape[1], y.shape[2])

    def run(self, srcs, frame_hw, **kw):
        """srcs: (B, L, C) sources viewed as (B, 1, L, C); frame_hw = (1, L)."""
        if self._taps():
            return self._run_taps(srcs, frame_hw, **kw)
        self._check()
        pk = self._packed(lambda w: ops.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1)), "conv1d")
        return ops.conv2d(srcs, frame_hw, pk, self.bias, self.out_channels, 1, 1, **kw)

    def run_ad(self, x):
        """Differentiable form: x (B, 1, L, Cin)."""
        if self._taps():
            return ad.conv1d(self, x)
        self._check()
        return ad.Conv2dFn.apply((1, 1, 1, 1, (0, 0), (0, 0), 0), x,
                                 self.weight.reshape(self.out_channels, self.in_channels, 1, 1), self.bias)


class ConvTranspose1d(_PackedMixin, nn.ConvTranspose1d):
    """nn.ConvTranspose1d(k=4, s=2, padding 0 or 1) parameters: the 1-D U-Net Upsample ('ones' mode) as the two 2-tap
    phase convs of nps_conv1d_fwd, on (B, 1, L, C) fp32 maps."""

    def run(self, x, act=0):
        ad.check_conv_transpose1d(self)
        if x.dim() != 4 or x.shape[1] != 1:
            raise RuntimeError(f"ConvTranspose1d.run: a (B, 1, L, C) map expected, got {tuple(x.shape)}")
        B, _, L, C = x.shape
        p = self.padding[0]
        phases = self._packed(lambda w: [ops.pack_conv1d_weight(q) for q in ops.conv_transpose1d_phase_weights(w)],
                              "convT1")
        out = torch.empty((B, 1, 2 * L + 2 - 2 * p, self.out_channels), dtype=torch.float32, device=x.device)
        for r in (0, 1):
            ops.conv1d([ops.Src(x)], L, phases[r], self.bias, self.out_channels, 2, pad=(1, 1), out=out[:, 0],
                       out_os=2, out_off=r - p, act=act)
        return out

    def run_ad(self, x):
        return ad.conv_transpose1d(self, x)

    def forward(self, x):
        """(B, C, L) -> (B, Cout, 2 L + 2 - 2 padding)."""
        form = AUTOGRAD1D if use_autograd(self) else INFER1D
        return form.to_out(form.upsample(self, form.to_in(x)))


def flat_frame(spatial):
    """The (rows, row length) arrangement of a grid's flat pixels that the per-pixel NHWC launches (pointwise convs,
    spectral layers) take: (1, L), (H, W) or (D*H, W).  Channels-last (B, N, C) tensors view to (B, rows, row, C)."""
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) == 1:
        return 1, spatial[0]
    if len(spatial) == 2:
        return spatial
    if len(spatial) == 3:
        return spatial[0] * spatial[1], spatial[2]
    raise NotImplementedError(f"grids have 1 to 3 spatial axes, got {len(spatial)}")


def run_pointwise(conv, srcs, out=None, **kw):
    """conv.run on the sources srcs (B, rows, row, C) of a pointwise conv (an FNO layer's (h | vb), an encoder's or
    decoder's one tensor).  A Conv1d's 1 x L image folds into 32-point rows when L % 32 == 0, L > 32 and no source is
    offset: a pointwise conv does not care how its pixels are arranged, and 32-point rows fill the 2-D conv tiles that
    a 1 x L image would leave 1/8 .. 1/32 used.  `out` (to write or accumulate into) and the result are in the
    sources' arrangement (planar with out_nchw=True, where the fold changes nothing)."""
    B, R, L = srcs[0].t.shape[:3]
    if not (isinstance(conv, Conv1d) and R == 1 and L % 32 == 0 and L > 32
            and all(s.off_y == 0 and s.off_x == 0 for s in srcs)):
        return conv.run(srcs, (R, L), out=out, **kw)
    fold = lambda t: ops.pixel_view(t, (B, L // 32, 32, t.shape[3]))  # noqa: E731
    y = conv.run([ops.Src(fold(s.t)) for s in srcs], (L // 32, 32), out=fold(out) if out is not None else None, **kw)
    if out is not None:
        return out
    return y.view(B, -1, 1, L) if kw.get("out_nchw") else ops.pixel_view(y, (B, 1, L, y.shape[3]))


def get_conv_with_right_spatial_dim(spatial_dim, **kwargs):
    """common.py:37-47."""
    if spatial_dim == 1:
        return Conv1d(**kwargs)
    if spatial_dim == 2:
        return Conv2d(**kwargs)
    if spatial_dim == 3:
        return Conv3d(**kwargs)
    raise NotImplementedError(f"only 0<x<=3d convs implemented so far, but found spatial dim {spatial_dim}!")


class ConvTranspose3d_padded(_Packed3Mixin, nn.ConvTranspose3d):
    """The 3-D U-Net Upsample, DEFINED by this build (the reference raises NotImplementedError for 3-D,
    common.py:103-120): the 2-D rule of ConvTranspose2d_padded (common.py:93-100) applied per axis —
    circular pad `pad` on every spatial axis, then ConvTranspose3d(k=4, s=2, p=0).  Runs as the 8 phase
    convs of nps_conv3d (transposed)."""

    def __init__(self, pad, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pad = pad

    def run3d(self, x, **kw):
        if (set(self.kernel_size) != {4} or set(self.stride) != {2} or set(self.padding) != {0}
                or set(self.output_padding) != {0} or set(self.dilation) != {1} or self.groups != 1):
            raise NotImplementedError("3-D Upsample: ConvTranspose3d(k=4, s=2, p=0) only")
        bf16 = x.dtype == torch.bfloat16
        return ops.conv3d([ops.Src3(x)], x.shape[1:4], self._packed3(bf16, transposed=True), self.bias,
                          self.out_channels, 2, transposed=True, circ=self.pad, zpad=1, **kw)

    def forward(self, x):
        if use_autograd(self) and x.dtype == torch.float32:
            return _ad_ncdhw(ad.conv_transpose3d, self, x)
        return run_form(self, x, None, lambda form, x, _: self.run3d(x))


def get_upconv_with_right_spatial_dim(spatial_dim, in_channels, out_channels, **kwargs):
    """common.py:103-120, plus a 3-D circular form the reference lacks (ConvTranspose3d_padded)."""
    if spatial_dim == 1:
        return ConvTranspose1d(in_channels, out_channels, **kwargs)
    if spatial_dim == 2:
        if kwargs.get("padding_mode") == "circular":
            kernel_size = kwargs["kernel_size"]
            slice_size = (kernel_size - 1) // 2
            kw = copy.deepcopy(kwargs)
            del kw["padding_mode"]
            return ConvTranspose2d_padded(slice_size, in_channels, out_channels, **kw)
        return ConvTranspose2d(in_channels, out_channels, **kwargs)
    if spatial_dim == 3 and kwargs.get("padding_mode") == "circular":
        # DESIGN.md "3-D U-FNO": BASELINE config C5 needs a 3-D Upsample; defined as the 2-D rule per axis
        kw = copy.deepcopy(kwargs)
        del kw["padding_mode"]
        return ConvTranspose3d_padded((kw["kernel_size"] - 1) // 2, in_channels, out_channels, **kw)
    raise NotImplementedError(f"only 0<x<=2d convs implemented so far, but found spatial dim {spatial_dim}!")


class Form(NamedTuple):
    """One of the four ways the U-Net modules run on channels-last activations."""
    run: str             # the per-module method: run / run_ad / run3d / run_ad3d
    Src: type            # ops.Src / ops.Src3
    nd: int              # spatial dims: a map's size is shape[1:1 + nd]
    upsample: Callable   # (Upsample.conv, h) -> the transposed conv's output
    to_in: Callable      # channels-first -> channels-last at a module boundary
    to_out: Callable     # and back
    dims: int = 0        # the num_spatial_dims of the models the form serves, when it is not nd (the 1-D forms)


def _upsample3d(conv, h):
    st = ops.new_stats(h.shape[0], h) if ops.CARRY3D else None  # (moments of the 8 phases' outputs)
    h = conv.run3d(h, out_stats=st)
    return h if st is None else ops.attach_stats(h, st)


INFER2D = Form("run", ops.Src, 2, lambda conv, h: conv.run(h), ops.nchw_to_nhwc, ops.nhwc_to_nchw)
AUTOGRAD2D = Form("run_ad", ops.Src, 2, ad.conv_transpose2d, ad.to_nhwc, ad.to_nchw)
INFER3D = Form("run3d", ops.Src3, 3, _upsample3d, to_ndhwc, to_ncdhw)
# fp32 training in 3-D.  run_form never picks it (the 3-D module boundaries refuse grad mode): UFNO.forward and the
# NDHWC methods run_ad3d are its entries.
AUTOGRAD3D = Form("run_ad3d", ops.Src3, 3, ad.conv_transpose3d, ad_to_ndhwc, ad_to_ncdhw)
# 1-D: (B, C, L) tensors walk as (B, 1, L, C) maps through the 2-D methods (frames, GroupNorm, attention); the convs
# and the Upsample are the modules' own run / run_ad (Conv1d, ConvTranspose1d).
INFER1D = Form("run", ops.Src, 2, lambda conv, h: conv.run(h), lambda x: ops.nchw_to_nhwc(x.unsqueeze(2)),
               lambda y: ops.nhwc_to_nchw(y).squeeze(2), 1)
AUTOGRAD1D = Form("run_ad", ops.Src, 2, lambda conv, h: conv.run_ad(h), lambda x: ad.to_nhwc(x.unsqueeze(2)),
                  lambda y: ad.to_nchw(y).squeeze(2), 1)


def form_dims(form):
    """The num_spatial_dims of the models a form serves."""
    return form.dims or form.nd


def run_form(mod, x, vb, fn):
    """The module boundary of a forward(): fn(form, x, vb) on the channels-last x and conditioning vb (or None) in
    the form that x and the grad mode call for; the tensor or tuple of tensors it returns, channels-first."""
    if x.dim() == 3:
        form = AUTOGRAD1D if use_autograd(mod) else INFER1D
    else:
        form = INFER3D if x.dim() == 5 else AUTOGRAD2D if use_autograd(mod) else INFER2D
    if form is INFER3D and use_autograd(mod):
        raise NotImplementedError("the 3-D U-Net is inference-only on the MI355X path (C5 rollout)")
    vb = form.to_in(vb) if vb is not None else None
    y = fn(form, form.to_in(x), vb)
    return tuple(form.to_out(t) for t in y) if isinstance(y, tuple) else form.to_out(y)


# bf16 storage (C5) of the 3-D FNO family's per-pixel layers: bf16 channels-last views through the fp32 transposes
# (an fp32 conditioning next to bf16 activations is converted as fp32); inference only
BF16FLAT = Form("run_bf16", ops.Src, 2, None,
                lambda t: ops.to_bf16(ops.nchw_to_nhwc(ops.to_f32(t) if t.dtype == torch.bfloat16 else t.float())),
                lambda y: ops.to_bf16(ops.nhwc_to_nchw(ops.to_f32(y))))


def run_flat(mod, x, vb, fn, bf16=False):
    """The module boundary of a per-pixel module's forward() (FNO layers, spectral and pointwise convs, and the U-FNO
    whose U-Nets walk the same maps) at every grid rank: fn(form, h, vb, spatial) on the channels-last
    (B, rows, row, C) views (flat_frame) of the (B, C, *spatial) tensor x and conditioning vb (or None), in the form
    that the grad mode calls for (INFER2D / AUTOGRAD2D; BF16FLAT for a bf16 x of a module with a bf16-storage form,
    `bf16`); the tensor it returns, as (B, C', *spatial)."""
    spatial = tuple(x.shape[2:])
    frame = flat_frame(spatial)
    form = BF16FLAT if (bf16 and x.dtype == torch.bfloat16) else AUTOGRAD2D if use_autograd(mod) else INFER2D
    # (a 2-D tensor goes in and comes out as it is: it keeps the range tag it carries)
    flat = lambda t: t if spatial == frame else t.reshape(t.shape[:2] + frame)  # noqa: E731
    vb = form.to_in(flat(vb)) if vb is not None else None
    y = form.to_out(fn(form, form.to_in(flat(x)), vb, spatial))
    return y if spatial == frame else y.reshape(y.shape[:2] + spatial)
