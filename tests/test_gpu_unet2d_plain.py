"""A 2-D norm=False, use1x1=True U-Net whose hidden channels are a multiple of 16: its final conv is a 1x1 conv with a
GELU prologue and no GroupNorm on 16-channel-aligned sources, the one launch the split-fp16 1x1 kernel's fused
prologue cannot take (it reads the GroupNorm affine for its input range); the host routes it through nps_frame_pack
(nps_conv2d_x3_prologue_ok).  Inference and autograd forward against an fp64 restatement of the same module tree with
torch's own ops on the CPU (F.conv2d / F.conv_transpose2d / F.gelu / torch.cat / F.pad as crop_Nd), rel-L2 < 1e-5, the
project's fp32 bar; 16 x 12 (no crop anywhere) and 13 x 10 (13 -> 7 -> 14, 10 -> 5 -> 10: the skip is padded into the
up frame and the output cropped)."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(num_spatial_dims=2, n_cond=2, hidden_features=16, ch_mults=[1, 2], n_blocks=1, norm=False,
          is_attn=[False, False], mid_attn=False, padding_mode="ones", use1x1=True)


def _crop(x, hw):
    """crop_Nd (reference common.py:20-34): per axis pad round(p - 0.001) in front, round(p + 0.001) behind"""
    pads = []
    for cur, des in zip(reversed(x.shape[2:]), reversed(hw)):
        p = (des - cur) / 2
        pads += [int(round(p - 0.001)), int(round(p + 0.001))]
    return F.pad(x, pads)


def _conv(m, x):
    w, b = m.weight.double(), m.bias.double()
    if isinstance(m, nn.ConvTranspose2d):
        return F.conv_transpose2d(x, w, b, stride=m.stride, padding=m.padding)
    return F.conv2d(x, w, b, stride=m.stride, padding=m.padding)


def _res(m, x):
    h = _conv(m.conv2, F.gelu(_conv(m.conv1, F.gelu(x))))
    sc = x if isinstance(m.shortcut, nn.Identity) else _conv(m.shortcut, x)
    return _crop(h, sc.shape[2:]) + sc


def _restated(m, h, vb):
    from models.enc_proc_dec_components.proc_unet_modern import Downsample, Upsample
    hw0 = h.shape[2:]
    feats, vbs = [h], [vb]
    for blk in m.down:
        if isinstance(blk, Downsample):
            h, vb = _conv(blk.conv, h), _conv(blk.conv_variables_broadcast, vb)
        else:
            h = _res(blk.res, torch.cat((h, vb), 1))
        feats.append(h)
        vbs.append(vb)
    h = _res(m.middle.res2, _res(m.middle.res1, torch.cat((h, vb), 1)))
    for blk in m.up:
        if isinstance(blk, Upsample):
            h = _conv(blk.conv, h)
        else:
            h = _res(blk.res, torch.cat((h, _crop(feats.pop(), h.shape[2:]), _crop(vbs.pop(), h.shape[2:])), 1))
    return _crop(_conv(m.final, F.gelu(h)), hw0)


@functools.lru_cache(maxsize=None)
def _case(hw):
    from models.enc_proc_dec_components import UNetModern
    torch.manual_seed(11)
    m = UNetModern(pde=None, activation=nn.GELU(), **KW)
    g = torch.Generator().manual_seed(12)
    x, vb = torch.rand(2, 16, *hw, generator=g) * 2 - 1, torch.rand(2, 2, *hw, generator=g) * 2 - 1
    with torch.no_grad():
        ref = _restated(m, x.double(), vb.double())
    return m.to(DEV), x, vb, ref


@pytest.mark.parametrize("hw", [(16, 12), (13, 10)])
def test_final_1x1_with_an_activation_only_prologue(hw):
    from nps_hip import lib
    assert lib.nps_conv2d_x3_prologue_ok(1, 1, 16, 0, 1) == 0  # (the launch is fed by nps_frame_pack)
    m, x, vb, ref = _case(hw)
    with torch.no_grad():
        y = m(x.to(DEV), vb.to(DEV))
    y_ad = m(x.to(DEV), vb.to(DEV))
    e, e_ad = rel_l2(y, ref), rel_l2(y_ad, ref)
    print(f"2-D plain U-Net {hw}: inference rel-L2 {e:.2e}, autograd form {e_ad:.2e}")
    assert y.shape == ref.shape and y_ad.requires_grad and e < 1e-5 and e_ad < 1e-5
