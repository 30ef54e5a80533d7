"""Modern U-Net (reference models/enc_proc_dec_components/proc_unet_modern.py).

Same module tree / kwargs / state_dict as the reference.  The forward is a
chain of fused HIP launches on NHWC tensors:
  * a ResidualBlock = GN-stats(x) -> conv1 [GN+GELU prologue] -> GN-stats ->
    conv2 [GN+GELU prologue] accumulated at the crop_Nd offset into the
    shortcut (1x1 conv or x);
  * torch.cat((h, crop_Nd(skip), crop_Nd(vb))) never exists: the three tensors
    are sources of one virtual conv input frame with their crop offsets;
  * the final GN(8)+GELU+conv+crop is one conv launch whose epilogue can also
    fuse the U-FNO `GELU(h_fno + h_unet)` (proc_ufno.py:118).

The model runs in four forms (models.common.Form): 2-D inference (`run`, the fused launches above), 2-D
autograd (`run_ad`, the same kernels unfused plus their backward kernels), 3-D inference (`run3d`, NDHWC) and 3-D
autograd (`run_ad3d`, NDHWC fp32).  A 1-D U-Net (padding_mode "ones": every conv zero-padded) walks (B, 1, L, C)
maps through the 2-D methods in the two 1-D forms: frames, GroupNorm and attention are the 2-D launches; its convs —
k-tap, the pointwise shortcuts and final conv (Conv1d.exact) — and its Upsample are Conv1d / ConvTranspose1d's own
run / run_ad (the Conv1d kernels that tile along L, exact fp32, no fused prologue and no carried moments).
The down / middle / up traversal is written once, `UNetModern._walk(form, h, vb)`, and so is each
Down / MiddleBlock body (`_run(form, x, vb)`); a form names the per-module method, the source tuple, the number
of spatial dims and how an Upsample is applied.  What differs by algorithm stays written per form: the three
ResidualBlock bodies, AttentionBlock, Downsample and the final conv stage of `UNetModern.run / run_ad / run3d /
run_ad3d`.  Every forward() enters through models.common.run_form, which picks the form, converts the layout in and
out and refuses 3-D under autograd: the 3-D autograd form is entered through UFNO.forward or by calling run_ad3d.
"""
from typing import List, Tuple, Union

import torch
from torch import nn

from common.interfaces import D, M
from models.common import (get_conv_with_right_spatial_dim, get_upconv_with_right_spatial_dim, crop_offsets,
                           activation_code, run_form, form_dims, INFER1D, AUTOGRAD1D, INFER2D, AUTOGRAD2D, INFER3D,
                           AUTOGRAD3D)
from nps_hip import ops
from nps_hip import autograd as ad
from pdes import PDE


def _gn_args(norm_mod, stats):
    return ops.GN(stats, norm_mod.weight, norm_mod.bias, norm_mod.num_groups, float(norm_mod.eps))


def _whole_frame(srcs, size):
    """True when the frame is one source covering it (x itself, not a concatenation or a placed crop)."""
    return len(srcs) == 1 and not any(srcs[0][1:]) and tuple(srcs[0].t.shape[1:1 + len(size)]) == tuple(size)


def _res_attn(form, m, res, srcs, size):
    """m.attn(res(frame of srcs)) of a Down / Middle / Up block m in the given form."""
    if isinstance(m.attn, nn.Identity):
        return getattr(res, form.run)(srcs, size)
    if form.nd == 3:
        raise NotImplementedError("3-D U-Net attention is not on the MI355X path")
    return getattr(m.attn, form.run)(getattr(res, form.run)(srcs, size))


class UNetModern(nn.Module):
    """proc_unet_modern.py:24-196."""
    model_interface = M.AR_TB
    data_interface = [D.sim1d, D.sim2d, D.sim1d_var_t]

    def __init__(self, pde: PDE, num_spatial_dims: int = 1, n_cond: int = 0, hidden_features: int = 128,
                 cond_mode: str = "concat", activation: nn.Module = nn.GELU(), norm: bool = False,
                 ch_mults: Union[Tuple[int, ...], List[int]] = (1, 2, 2, 4),
                 is_attn: Union[Tuple[bool, ...], List[bool]] = (False, False, False, False), mid_attn: bool = False,
                 n_blocks: int = 2, use1x1: bool = False, padding_mode: str = "ones", **kwargs) -> None:
        super().__init__()
        self.hidden_features = hidden_features
        self.num_spatial_dims = num_spatial_dims
        assert cond_mode in ["concat", None], "Incorrect conditioning mode supplied"
        self.cond_mode = cond_mode
        self.n_cond = 0 if self.cond_mode is None else n_cond
        assert padding_mode in ["ones", "circular"]
        self.padding_mode = padding_mode
        padding_kwargs = dict(padding=1) if padding_mode == "ones" else dict(padding_mode="circular")
        self.activation: nn.Module = activation
        n_resolutions = len(ch_mults)
        n_channels = hidden_features
        down = []
        out_channels = in_channels = n_channels
        for i in range(n_resolutions):
            out_channels = in_channels * ch_mults[i]
            for _ in range(n_blocks):
                down.append(DownBlock(in_channels + n_cond, out_channels, has_attn=is_attn[i], activation=activation,
                                      norm=norm, num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs))
                in_channels = out_channels
            if i < n_resolutions - 1:
                down.append(Downsample(in_channels, num_spatial_dims=num_spatial_dims, n_cond=n_cond,
                                       padding_kwargs=padding_kwargs))
        self.down = nn.ModuleList(down)
        self.middle = MiddleBlock(in_channels=out_channels + n_cond, out_channels=out_channels, has_attn=mid_attn,
                                  activation=activation, norm=norm, num_spatial_dims=num_spatial_dims,
                                  padding_kwargs=padding_kwargs)
        up = []
        in_channels = out_channels
        for i in reversed(range(n_resolutions)):
            out_channels = in_channels
            for _ in range(n_blocks):
                up.append(UpBlock(in_channels + n_cond, out_channels, has_attn=is_attn[i], activation=activation,
                                  norm=norm, num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs))
            out_channels = in_channels // ch_mults[i]
            up.append(UpBlock(in_channels + n_cond, out_channels, has_attn=is_attn[i], activation=activation,
                              norm=norm, num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs))
            in_channels = out_channels
            if i > 0:
                up.append(Upsample(in_channels, num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs))
        self.up = nn.ModuleList(up)
        self.norm = nn.GroupNorm(8, n_channels) if norm else nn.Identity()
        if use1x1:
            self.final = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                                         out_channels=hidden_features, kernel_size=1)
        else:
            self.final = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=hidden_features,
                                                         out_channels=hidden_features, kernel_size=3, **padding_kwargs)
        if num_spatial_dims == 1:
            self.final.exact = True  # (a pointwise final conv on the exact-fp32 Conv1d kernels: models.common.Conv1d)

    def _walk(self, form, h, vb):
        """Down, middle and up (proc_unet_modern.py:169-193) in the given form.  Returns the last feature map and the
        input's shape (the final conv's crop target)."""
        if self.num_spatial_dims != form_dims(form):
            raise NotImplementedError("UNetModern: 2-D only on the MI355X path" if form.nd == 2 else
                                      "UNetModern.run3d: 3-D U-Nets only")
        if self.num_spatial_dims == 1:
            self.check_1d()
        if self.n_cond > 0 and vb is None:
            # reference Downsample.forward returns a bare tensor here (proc_unet_modern.py:451-455) which
            # :175 then unpacks along the batch dimension; refuse instead of reproducing that bug
            raise ValueError("UNetModern with n_cond > 0 needs variables_broadcast")
        if self.n_cond == 0:
            vb = None
        h_shape, sp = h.shape, slice(1, 1 + form.nd)
        feats, vbs = [h], [vb]
        for m in self.down:
            if isinstance(m, Downsample):
                h, vb = getattr(m, form.run)(h, vb)
            else:
                h = m._run(form, h, vb)
            feats.append(h)
            vbs.append(vb)
        h = self.middle._run(form, h, vb)
        for m in self.up:
            if isinstance(m, Upsample):
                h = form.upsample(m.conv, h)
            else:
                # cat((h, crop_Nd(skip), crop_Nd(vb))) as the three sources of one frame
                s, v, size = feats.pop(), vbs.pop(), tuple(h.shape[sp])
                srcs = [form.Src(h), form.Src(s, *crop_offsets(s.shape[sp], size))]
                if v is not None:
                    srcs.append(form.Src(v, *crop_offsets(v.shape[sp], size)))
                h = _res_attn(form, m, m.res, srcs, size)
        return h, h_shape

    def check_1d(self):
        """The 1-D U-Net on the HIP path is the zero-padded one."""
        if self.padding_mode != "ones":
            raise NotImplementedError(
                f"UNetModern: the 1-D HIP path is the zero-padded padding_mode='ones' U-Net, got "
                f"{self.padding_mode!r} (the reference cannot build a circular 1-D U-Net of more than one level: "
                "nn.ConvTranspose1d takes zero padding only)")

    def run(self, h, vb, addend=None, act_after=0, addend_fork=None):
        """NHWC forward (proc_unet_modern.py:169-196).  Optional fused epilogue on the final conv:
        out = act_after(final(...) + addend) — the U-FNO block combination.  addend_fork: the ops.Fork whose
        side stream computes addend (joined just before the final conv)."""
        h, h_shape = self._walk(INFER1D if self.num_spatial_dims == 1 else INFER2D, h, vb)
        # final: conv(act(norm(h))) then crop_Nd to the input size, as one launch
        H, W = h.shape[1:3]
        gn = None
        if isinstance(self.norm, nn.GroupNorm):
            gn = _gn_args(self.norm, ops.group_norm_stats([ops.Src(h)], (H, W), self.norm.num_groups))
        oy, ox = crop_offsets(self.final.out_hw(H, W), h_shape[1:3])
        B, Ht, Wt = h_shape[0], h_shape[1], h_shape[2]
        if addend_fork is not None:
            addend_fork.join(addend)
        out = ops.empty_nhwc(B, Ht, Wt, self.final.out_channels, h)
        border = oy > 0 or ox > 0
        if border:
            out.zero_()  # crop_Nd zero-pads when the output is smaller than the input
        # the conv epilogue adds the addend and applies act_after only where it stores: with a zero-padded border
        # (a single-resolution circular U-Net with a 3x3 final conv) the border must still become
        # act_after(addend + 0), so that geometry takes the unfused add-then-activate of run_ad
        unfused = border and addend is not None
        # the output carries its GroupNorm(1) moments (the next U-FNO block's norm1 frame reads it): no statistics
        # pass over it (zero crop padding adds nothing to the sums)
        st = ops.new_stats(B, out)
        self.final.run([ops.Src(h)], (H, W), gn=gn, pre_act=activation_code(self.activation), out=out,
                       out_off=(oy, ox), addends=[addend] if addend is not None and not unfused else [],
                       act=0 if unfused else act_after, out_stats=st)
        if unfused:  # (a new tensor: it carries no moments, the next norm1 takes them in a statistics pass)
            with torch.no_grad():
                return ad.act(ad.add_at(addend, out), act_after)
        return ops.attach_stats(out, st)

    def run_ad(self, h, vb):
        """Differentiable NHWC forward (training): proc_unet_modern.py:169-196 as unfused HIP ops."""
        h, h_shape = self._walk(AUTOGRAD1D if self.num_spatial_dims == 1 else AUTOGRAD2D, h, vb)
        norm = self.norm if isinstance(self.norm, nn.GroupNorm) else None
        y = self.final.run_ad(ad.frame([ops.Src(h)], h.shape[1:3], norm, activation_code(self.activation)))
        return ad.crop(y, h_shape[1:3], crop_offsets(y.shape[1:3], h_shape[1:3]))

    def run3d(self, h, vb, addend=None, act_after=0, addend_fork=None):
        """NDHWC forward of the 3-D U-Net (proc_unet_modern.py:169-196 with num_spatial_dims=3; the 3-D
        Upsample is this build's ConvTranspose3d_padded), fp32 or bf16 storage.  Optional fused epilogue on
        the final conv: out = act_after(final(...) + addend) — the U-FNO block combination."""
        h, h_shape = self._walk(INFER3D, h, vb)
        dhw = tuple(h.shape[1:4])
        gn = None
        if isinstance(self.norm, nn.GroupNorm):
            gn = _gn_args(self.norm, ops.gn_stats3d([ops.Src3(h)], dhw, self.norm.num_groups))
        off = crop_offsets(self.final.out_dhw(dhw), h_shape[1:4])
        if addend_fork is not None:
            addend_fork.join(addend)
        out = torch.empty(tuple(h_shape[:4]) + (self.final.out_channels,), dtype=h.dtype, device=h.device)
        border = any(o > 0 for o in off)
        if border:
            out.zero_()  # crop_Nd zero-pads when the output is smaller than the input
        # as run(): a zero-padded border under a fused addend must become act_after(addend + 0), which the conv
        # epilogue (it touches only what it stores) cannot give: the unfused add-then-activate of run_ad3d
        unfused = border and addend is not None
        if unfused and out.dtype != torch.float32:
            raise NotImplementedError("UNetModern.run3d: a final conv smaller than its input under a fused addend "
                                      "(single-resolution circular U-FNO, use1x1=False) runs in fp32 storage only")
        # the output's moments (the next U-FNO block's first norm1): those of the values the final conv stores
        # (after the addend and act_after; the crop border stays zero)
        st = ops.new_stats(out.shape[0], out) if ops.CARRY3D else None
        self.final.run3d([ops.Src3(h)], dhw, gn=gn, pre_act=activation_code(self.activation), out=out, out_off=off,
                         addend=None if unfused else addend, act=0 if unfused else act_after, out_stats=st)
        if unfused:  # (a new tensor without moments: the next norm1 takes them in a statistics pass)
            with torch.no_grad():
                return ad.act(ad.add_at3d(addend, out), act_after)
        if st is not None:
            ops.attach_stats(out, st)
        return out

    def run_ad3d(self, h, vb):
        """Differentiable NDHWC fp32 forward of the 3-D U-Net (training): run3d() as unfused HIP ops."""
        h, h_shape = self._walk(AUTOGRAD3D, h, vb)
        norm = self.norm if isinstance(self.norm, nn.GroupNorm) else None
        y = ad.conv3d(self.final, ad.frame3d([ops.Src3(h)], h.shape[1:4], norm, activation_code(self.activation)))
        return ad.crop3d(y, h_shape[1:4], crop_offsets(y.shape[1:4], h_shape[1:4]))

    def forward(self, h: torch.Tensor, variables_broadcast: torch.Tensor = None, pos=None):
        assert h.dim() == 2 + self.num_spatial_dims
        if self.num_spatial_dims == 1:
            self.check_1d()  # a circular 1-D U-Net raises before any work
        return run_form(self, h, variables_broadcast, lambda form, h, vb: getattr(self, form.run)(h, vb))


class ResidualBlock(nn.Module):
    """proc_unet_modern.py:199-250."""

    def __init__(self, in_channels: int, out_channels: int, activation: nn.Module = torch.nn.GELU(),
                 norm: bool = False, n_groups: int = 1, num_spatial_dims: int = 1, padding_kwargs: dict = None):
        super().__init__()
        self.activation: nn.Module = activation
        padding_kwargs = padding_kwargs or dict()
        self.conv1 = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=in_channels,
                                                     out_channels=out_channels, kernel_size=3, **padding_kwargs)
        self.conv2 = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=out_channels,
                                                     out_channels=out_channels, kernel_size=3, **padding_kwargs)
        if in_channels != out_channels:
            self.shortcut = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=in_channels,
                                                            out_channels=out_channels, kernel_size=1)
            if num_spatial_dims == 1:
                self.shortcut.exact = True  # (on the exact-fp32 Conv1d kernels: models.common.Conv1d)
        else:
            self.shortcut = nn.Identity()
        if norm:
            self.norm1 = nn.GroupNorm(n_groups, in_channels)
            self.norm2 = nn.GroupNorm(n_groups, out_channels)
        else:
            self.norm1 = nn.Identity()
            self.norm2 = nn.Identity()
        self.num_spatial_dims = num_spatial_dims

    def _shortcut_fork(self, srcs, H, W):
        """An ops.Fork for the shortcut when conv1's launch leaves >= SIDE_MIN_IDLE of the CUs idle in its
        last round (the 258^2 convs: 1122 tiles on 256 CUs at B = 2), else None (no fork: cross-stream waits
        cost more than an exact-round launch leaves idle)."""
        x0 = srcs[0].t
        if not (x0.is_cuda and ops.SIDE_STREAM):
            return None
        idle = ops.last_round_idle(*self.conv1.out_hw(H, W), x0.shape[0], self.conv1.out_channels, x0.device,
                                   Cin=sum(s.t.shape[3] for s in srcs))
        return ops.Fork(x0, settle=[s.t for s in srcs]) if idle >= ops.SIDE_MIN_IDLE else None

    def run(self, srcs, frame_hw):
        """srcs: the virtual NHWC input x (concat of slices).  Returns crop_Nd(h, sc) + sc."""
        act = activation_code(self.activation)
        H, W = frame_hw
        gn1 = gn2 = None
        if isinstance(self.norm1, nn.GroupNorm):
            gn1 = _gn_args(self.norm1, ops.group_norm_stats(srcs, (H, W), self.norm1.num_groups))
        # The block output's moments (the next block's norm1): those of the shortcut output — x's own for
        # the identity, else added by the 1x1 conv — then conv2, accumulating at its crop offset, adds
        # the change it makes (nps_conv2d_t.out_stats)
        st2 = out = None
        fork = None
        if isinstance(self.shortcut, nn.Identity):
            if _whole_frame(srcs, frame_hw):
                x = srcs[0].t
                out = ops.share_tag(x.clone(), x)  # conv2 accumulates into it: same bound
            else:
                # in_channels (with the conditioning / skip channels) == out_channels: the identity adds the
                # concatenation itself (e.g. hidden 16 + n_cond 16 -> 32), materialised once by nps_frame_pack
                out = x = ops.frame_pack(srcs, frame_hw)
            if isinstance(self.norm1, nn.GroupNorm):
                st2 = ops.copy_stats(ops.source_stats(x))
        else:
            # the 1x1 shortcut reads only x: it runs on a side stream beside conv1 (ops.Fork) when conv1's
            # persistent grid leaves many CUs idle in its last round (the 258^2 convs), its work-groups
            # taking them; its moments buffer is taken before the fork point (no fill on the side stream)
            st2 = ops.new_stats(srcs[0].t.shape[0], srcs[0].t) if isinstance(self.norm1, nn.GroupNorm) else None
            fork = self._shortcut_fork(srcs, H, W)
            if fork is None:
                out = self.shortcut.run(srcs, (H, W), out_stats=st2)
        # conv1 adds norm2's moments of h1 as it stores it (ops.conv2d out_stats): no statistics pass
        st1 = ops.new_stats(srcs[0].t.shape[0], srcs[0].t) if isinstance(self.norm2, nn.GroupNorm) else None
        h1 = self.conv1.run(srcs, (H, W), gn=gn1, pre_act=act, out_stats=st1)
        if st1 is not None:
            ops.attach_stats(h1, st1)
        if fork is not None:
            with fork:
                out = self.shortcut.run(srcs, (H, W), out_stats=st2)
        H1, W1 = h1.shape[1:3]
        if isinstance(self.norm2, nn.GroupNorm):
            gn2 = _gn_args(self.norm2, ops.group_norm_stats([ops.Src(h1)], (H1, W1), self.norm2.num_groups))
        if fork is not None:
            fork.join(out)  # conv2 accumulates into the shortcut output
        self.conv2.run([ops.Src(h1)], (H1, W1), gn=gn2, pre_act=act, out=out, accumulate=True, out_stats=st2,
                       out_off=crop_offsets(self.conv2.out_hw(H1, W1), out.shape[1:3]))
        if st2 is not None:
            ops.attach_stats(out, st2)
        return out

    def run3d(self, srcs, frame_dhw):
        """3-D form of run() on NDHWC Src3 sources: GN-stats -> conv1 [GN+GELU prologue] -> GN-stats ->
        conv2 [GN+GELU prologue] accumulated at the crop_Nd offset into the shortcut (1x1 conv or x)."""
        act = activation_code(self.activation)
        gn1 = gn2 = None
        if isinstance(self.norm1, nn.GroupNorm):
            # GroupNorm(1) of a frame of carried-moment sources: their sum, no pass (ops.group_norm_stats3d)
            gn1 = _gn_args(self.norm1, ops.group_norm_stats3d(srcs, frame_dhw, self.norm1.num_groups))
        # conv1 adds the moments of what it stores (nps_conv3d_t.out_stats): norm2's GroupNorm(1) statistics
        # without a pass over h1
        B = srcs[0].t.shape[0]
        carry = isinstance(self.norm2, nn.GroupNorm) and self.norm2.num_groups == 1
        st1 = ops.new_stats(B, srcs[0].t) if carry else None
        h1 = self.conv1.run3d(srcs, frame_dhw, gn=gn1, pre_act=act, out_stats=st1)
        # the block output's moments (the next block's norm1): the shortcut output's — x's own for the identity,
        # else added by the 1x1x1 conv — plus the change conv2 makes accumulating into it (as the 2-D run())
        carry_out = ops.CARRY3D and isinstance(self.norm1, nn.GroupNorm)
        st_out = None
        if isinstance(self.shortcut, nn.Identity):
            if _whole_frame(srcs, frame_dhw):
                out = srcs[0].t.clone()
                if carry_out:
                    st_out = ops.copy_stats(ops.source_stats3d(srcs[0].t))
            elif srcs[0].t.dtype != torch.float32:
                raise NotImplementedError("ResidualBlock.run3d: an identity shortcut on a concatenated input "
                                          "(in_channels with the conditioning / skip channels == out_channels) runs "
                                          "in fp32 storage only")
            else:
                # in_channels (with the conditioning / skip channels) == out_channels: the identity adds the
                # concatenation itself (e.g. hidden 16 + n_cond 16 -> 32), materialised once by nps_frame3d_fwd
                out = ops.frame3d(srcs, frame_dhw)
                if carry_out:
                    # the frame's moments are the sum of its sources' (zero crop padding adds nothing), as norm1
                    # took them above: the next norm1 needs no pass
                    st_out = ops.copy_stats(ops.group_norm_stats3d(srcs, frame_dhw, 1))
        else:
            st_out = ops.new_stats(B, srcs[0].t) if carry_out else None
            out = self.shortcut.run3d(srcs, frame_dhw, out_stats=st_out)
        d1 = tuple(h1.shape[1:4])
        if isinstance(self.norm2, nn.GroupNorm):
            st2 = (ops._stats_sum([st1], B, ops.new_stats(B, h1, 1)) if carry
                   else ops.gn_stats3d([ops.Src3(h1)], d1, self.norm2.num_groups))
            gn2 = _gn_args(self.norm2, st2)
        self.conv2.run3d([ops.Src3(h1)], d1, gn=gn2, pre_act=act, out=out, accumulate=True, out_stats=st_out,
                         out_off=crop_offsets(self.conv2.out_dhw(d1), out.shape[1:4]))
        if st_out is not None:
            ops.attach_stats(out, st_out)
        return out

    def run_ad(self, srcs, frame_hw):
        """Differentiable form of run(): frame -> GN+GELU -> conv1 -> GN+GELU -> conv2, + shortcut."""
        act = activation_code(self.activation)
        H, W = frame_hw
        n1 = self.norm1 if isinstance(self.norm1, nn.GroupNorm) else None
        n2 = self.norm2 if isinstance(self.norm2, nn.GroupNorm) else None
        # conv1's frame and the shortcut's input (x itself for the identity) from one node: the backward adds the
        # shortcut path's gradient inside the frame backward (ad.frame_pair), not as a separate accumulation
        f1, xin = ad.frame_pair(srcs, (H, W), n1, act) if ad.FRAME_PAIR else (ad.frame(srcs, (H, W), n1, act), None)
        h1 = self.conv1.run_ad(f1)
        if isinstance(self.shortcut, nn.Identity):
            sc = xin if xin is not None else ad.frame(srcs, (H, W))  # (x itself, or the concatenation)
        else:
            sc = self.shortcut.run_ad(xin if xin is not None else ad.frame(srcs, (H, W)))
        h2 = self.conv2.run_ad(ad.frame([ops.Src(h1)], h1.shape[1:3], n2, act))
        return ad.add_at(sc, h2, crop_offsets(h2.shape[1:3], sc.shape[1:3]))

    def run_ad3d(self, srcs, frame_dhw):
        """run_ad() in 3-D on NDHWC fp32 Src3 sources: frame pair -> conv1 -> frame -> conv2, added into the
        shortcut at its crop_Nd offset."""
        act = activation_code(self.activation)
        n1 = self.norm1 if isinstance(self.norm1, nn.GroupNorm) else None
        n2 = self.norm2 if isinstance(self.norm2, nn.GroupNorm) else None
        f1, xin = ad.frame_pair3d(srcs, frame_dhw, n1, act)
        h1 = ad.conv3d(self.conv1, f1)
        # (the identity adds x itself, or the plain concatenation the frame pair materialised)
        sc = xin if isinstance(self.shortcut, nn.Identity) else ad.conv3d(self.shortcut, xin)
        h2 = ad.conv3d(self.conv2, ad.frame3d([ops.Src3(h1)], h1.shape[1:4], n2, act))
        return ad.add_at3d(sc, h2, crop_offsets(h2.shape[1:4], sc.shape[1:4]))

    def forward(self, x: torch.Tensor):
        return run_form(self, x, None, lambda form, x, _: getattr(self, form.run)(
            [form.Src(x)], x.shape[1:1 + form.nd]))


_GEO_1X1 = (1, 1, 1, 1, (0, 0), (0, 0), 0)  # Conv2d.geometry() of a 1x1 conv


def _conv_weight(mod):
    """The weight of an nn.Linear / kernel-1 nn.Conv1d / 1x1 Conv2d as a (out, in, 1, 1) conv weight.  A Linear or
    Conv1d weight is viewed, not copied (gradients reach the parameter through the view); the fresh view shares
    one packing cache kept on the module, so ops.cached_pack packs it once per parameter version."""
    w = mod.weight
    if w.dim() == 4:
        return w
    if w.dim() == 3 and w.shape[2] != 1:
        raise NotImplementedError("attention shortcut: kernel-1 conv only")
    w4 = w.view(w.shape[0], w.shape[1], 1, 1)
    w4._nps_packs = mod.__dict__.setdefault("_nps_packs_1x1", {})
    return w4


def _run_1x1(mod, x, **kw):
    """mod (Linear / kernel-1 conv) applied per position of the NHWC map x on the fused 1x1 conv path."""
    w4 = _conv_weight(mod)
    pk = ops.cached_pack(w4, ("conv", 1, 1), lambda w: ops.pack_conv_weight(w, 1, 1))
    return ops.conv2d([ops.Src(x)], x.shape[1:3], pk, mod.bias, w4.shape[0], 1, 1, **kw)


def _run_1x1_ad(mod, x):
    return ad.Conv2dFn.apply(_GEO_1X1, x, _conv_weight(mod), mod.bias)


class AttentionBlock(nn.Module):
    """proc_unet_modern.py:253-317.  Tokens are the flattened positions of the map; `norm` exists as parameters
    and is never applied (:292-317 do not call it), so it stays in the state_dict and receives no gradient.  The
    softmax runs over the QUERY index for each key (:304, dim=1).  On NHWC maps the token-major [B, N, C] view is
    the map itself: `projection` and `output` run as 1x1 convs, the attention itself on nps_attn_* (no N x N
    scores), and `output`'s epilogue adds the shortcut.  The reference's forward only runs with one head and the
    identity shortcut (`res.view` at :308 needs a contiguous einsum result; :313 hands the shortcut conv the
    token-major view); more heads and the kernel-1 shortcut conv are computed here as those lines intend."""

    def __init__(self, in_channels: int, out_channels: int = None, n_heads: int = 1, d_k=None, n_groups: int = 1,
                 num_spatial_dims: int = 1):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        d_k = in_channels if d_k is None else d_k
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm = nn.GroupNorm(n_groups, in_channels)
        self.projection = nn.Linear(in_channels, n_heads * d_k * 3)
        self.output = nn.Linear(n_heads * d_k, out_channels)
        self.scale = d_k ** -0.5
        self.n_heads, self.d_k = n_heads, d_k
        if in_channels != out_channels:
            self.shortcut = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=in_channels,
                                                            out_channels=out_channels, kernel_size=1)
        else:
            self.shortcut = nn.Identity()

    def run(self, x):
        """NHWC inference forward.  x is only read (its producer's other consumers still use it); the result is a
        new tensor carrying its own GroupNorm(1) moments (or none, when the launch cannot take them: the next
        norm1 then runs a statistics pass) — never x's."""
        B, H, W, _ = x.shape
        qkv = _run_1x1(self.projection, x)
        o, _ = ops.attention(qkv.view(B, H * W, -1), self.n_heads, self.d_k, self.scale)
        sc = x if isinstance(self.shortcut, nn.Identity) else _run_1x1(self.shortcut, x)
        st = ops.new_stats(B, x)
        y = _run_1x1(self.output, o.view(B, H, W, -1), addends=[sc], out_stats=st)
        return ops.attach_stats(y, st)

    def run_ad(self, x):
        """Differentiable NHWC forward (training): the same launches unfused, gradients through Conv2dFn (the
        projections) and nps_attn_bwd."""
        B, H, W, _ = x.shape
        qkv = _run_1x1_ad(self.projection, x)
        o = ad.attention(qkv.view(B, H * W, -1), self.n_heads, self.d_k, self.scale)
        y = _run_1x1_ad(self.output, o.view(B, H, W, -1))
        sc = x if isinstance(self.shortcut, nn.Identity) else _run_1x1_ad(self.shortcut, x)
        return ad.add_at(sc, y)

    def forward(self, x: torch.Tensor):
        if x.dim() not in (3, 4):
            raise NotImplementedError("U-Net attention: 1-D and 2-D maps only on the MI355X path")
        return run_form(self, x, None, lambda form, x, _: getattr(self, form.run)(x))


def _frame(form, x, vb):
    """cat((x, vb)) as the sources of one frame."""
    return [form.Src(x)] + ([form.Src(vb)] if vb is not None else [])


class DownBlock(nn.Module):
    """proc_unet_modern.py:320-354."""

    def __init__(self, in_channels: int, out_channels: int, has_attn: bool = False, activation: nn.Module = nn.GELU(),
                 norm: bool = False, num_spatial_dims: int = 1, padding_kwargs: dict = None):
        super().__init__()
        self.res = ResidualBlock(in_channels, out_channels, activation=activation, norm=norm,
                                 num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs)
        self.attn = AttentionBlock(out_channels, num_spatial_dims=num_spatial_dims) if has_attn else nn.Identity()

    def _run(self, form, x, vb):
        return _res_attn(form, self, self.res, _frame(form, x, vb), x.shape[1:1 + form.nd])

    def forward(self, x: torch.Tensor, variables_broadcast: torch.Tensor = None):
        return run_form(self, x, variables_broadcast, self._run), variables_broadcast


class UpBlock(nn.Module):
    """proc_unet_modern.py:357-391."""

    def __init__(self, in_channels: int, out_channels: int, has_attn: bool = False, activation: nn.Module = nn.GELU(),
                 norm: bool = False, num_spatial_dims: int = 1, padding_kwargs: dict = None):
        super().__init__()
        self.res = ResidualBlock(in_channels + out_channels, out_channels, activation=activation, norm=norm,
                                 num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs)
        self.attn = AttentionBlock(out_channels, num_spatial_dims=num_spatial_dims) if has_attn else nn.Identity()

    def forward(self, x: torch.Tensor):
        return run_form(self, x, None, lambda form, x, _: _res_attn(
            form, self, self.res, [form.Src(x)], x.shape[1:1 + form.nd]))


class MiddleBlock(nn.Module):
    """proc_unet_modern.py:394-422."""

    def __init__(self, in_channels, out_channels: int, has_attn: bool = False, activation: nn.Module = nn.GELU(),
                 norm: bool = False, num_spatial_dims: int = 1, padding_kwargs: dict = None):
        super().__init__()
        self.res1 = ResidualBlock(in_channels, out_channels, activation=activation, norm=norm,
                                  num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs)
        self.attn = AttentionBlock(out_channels, num_spatial_dims=num_spatial_dims) if has_attn else nn.Identity()
        self.res2 = ResidualBlock(out_channels, out_channels, activation=activation, norm=norm,
                                  num_spatial_dims=num_spatial_dims, padding_kwargs=padding_kwargs)

    def _run(self, form, x, vb):
        h = _res_attn(form, self, self.res1, _frame(form, x, vb), x.shape[1:1 + form.nd])
        return getattr(self.res2, form.run)([form.Src(h)], h.shape[1:1 + form.nd])

    def forward(self, x: torch.Tensor, variables_broadcast: torch.Tensor = None):
        return run_form(self, x, variables_broadcast, self._run), variables_broadcast


class Upsample(nn.Module):
    """proc_unet_modern.py:425-436 (ConvTranspose2d k=4 s=2, circularly pre-padded in 'circular' mode)."""

    def __init__(self, n_channels: int, num_spatial_dims: int, padding_kwargs: dict):
        super().__init__()
        self.conv = get_upconv_with_right_spatial_dim(num_spatial_dims, in_channels=n_channels,
                                                      out_channels=n_channels, kernel_size=4, stride=2,
                                                      **padding_kwargs)

    def forward(self, x: torch.Tensor):
        return self.conv(x)


class Downsample(nn.Module):
    """proc_unet_modern.py:439-455 (3x3 stride-2 conv on h and on the conditioning channels)."""

    def __init__(self, n_channels: int, num_spatial_dims: int, n_cond: int, padding_kwargs: dict):
        super().__init__()
        self.conv = get_conv_with_right_spatial_dim(num_spatial_dims, in_channels=n_channels, out_channels=n_channels,
                                                    kernel_size=3, stride=2, **padding_kwargs)
        if n_cond > 0:
            self.conv_variables_broadcast = get_conv_with_right_spatial_dim(
                num_spatial_dims, in_channels=n_cond, out_channels=n_cond, kernel_size=3, stride=2, **padding_kwargs)

    def run(self, x, vb):
        st = ops.new_stats(x.shape[0], x)  # the next ResidualBlock's norm1 moments of h
        h = ops.attach_stats(self.conv.run([ops.Src(x)], x.shape[1:3], out_stats=st), st)
        if vb is not None:
            vb = self.conv_variables_broadcast.run([ops.Src(vb)], vb.shape[1:3])
        return h, vb

    def run_ad(self, x, vb):
        h = self.conv.run_ad(x)
        if vb is not None:
            vb = self.conv_variables_broadcast.run_ad(vb)
        return h, vb

    def run3d(self, x, vb):
        st = ops.new_stats(x.shape[0], x) if ops.CARRY3D else None  # the next ResidualBlock's norm1 moments of h
        h = self.conv.run3d([ops.Src3(x)], x.shape[1:4], out_stats=st)
        if st is not None:
            ops.attach_stats(h, st)
        if vb is not None:
            vb = self.conv_variables_broadcast.run3d([ops.Src3(vb)], vb.shape[1:4])
        return h, vb

    def run_ad3d(self, x, vb):
        h = ad.conv3d(self.conv, x)
        if vb is not None:
            vb = ad.conv3d(self.conv_variables_broadcast, vb)
        return h, vb

    def forward(self, x: torch.Tensor, variables_broadcast: torch.Tensor = None):
        if variables_broadcast is None:
            return self.conv(x)
        return run_form(self, x, variables_broadcast, lambda form, x, vb: getattr(self, form.run)(x, vb))
