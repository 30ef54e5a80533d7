"""Host checks of the geometry helpers the U-Net walk shares (models/common.py): crop_offsets for any rank,
Conv2d.out_hw and Conv3d.out_dhw against the shapes torch's own convolutions produce.  No GPU: the mirror's
forward is never called, only nn.Conv2d.forward / nn.Conv3d.forward on CPU tensors."""
import itertools

import pytest
import torch
from torch import nn

from models.common import Conv2d, Conv3d, crop_offsets


def _crop_ref(cur, des):
    return int(round((des - cur) / 2 - 0.001))


def test_crop_offsets_any_rank():
    pairs = list(itertools.product(range(1, 13), repeat=2))  # every (cur, des) in 1..12, on every axis
    for (c0, d0), (c1, d1) in itertools.product(pairs, repeat=2):
        assert crop_offsets((c0, c1), (d0, d1)) == (_crop_ref(c0, d0), _crop_ref(c1, d1))
    for i in range(len(pairs)):
        cur, des = zip(pairs[i], pairs[(i + 37) % len(pairs)], pairs[(i + 91) % len(pairs)])
        want = tuple(_crop_ref(c, d) for c, d in zip(cur, des))
        assert crop_offsets(cur, des) == want
        assert crop_offsets(torch.Size(cur), list(des)) == want


def _torch_shape(fwd, m, x):
    """Spatial shape of torch's own forward, or None where torch refuses the frame (kernel extent past the padded
    input)."""
    try:
        return tuple(fwd(m, x).shape[2:])
    except RuntimeError:
        return None


@pytest.mark.parametrize("padding_mode", ["zeros", "circular"])
@pytest.mark.parametrize("padding", [0, 1, "same", "valid"])
def test_conv2d_out_hw_is_torchs(padding, padding_mode):
    for k, s, d in itertools.product((1, 3, 5), (1, 2), (1, 2)):
        if padding == "same" and s != 1:
            continue  # torch: 'same' needs stride 1
        m = Conv2d(1, 1, k, stride=s, dilation=d, padding=padding, padding_mode=padding_mode)
        for H, W in itertools.product(range(6, 14), repeat=2):
            want = _torch_shape(nn.Conv2d.forward, m, torch.zeros(1, 1, H, W))
            got = m.out_hw(H, W)
            if want is None:  # only the 9-wide extent of k = 5, d = 2 can exceed a frame here
                assert d * (k - 1) + 1 > 6 and min(got) <= 0, (k, s, d, H, W, got)
            else:
                assert got == want, (k, s, d, H, W)


@pytest.mark.parametrize("padding_mode", ["zeros", "circular"])
@pytest.mark.parametrize("padding", [0, 1, "same", "valid"])
def test_conv3d_out_dhw_is_torchs(padding, padding_mode):
    for k, s in itertools.product((1, 3), (1, 2)):
        if padding == "same" and s != 1:
            continue
        m = Conv3d(1, 1, k, stride=s, padding=padding, padding_mode=padding_mode)
        for dhw in [(6, 7, 8), (13, 6, 9), (8, 8, 8), (7, 12, 11), (10, 13, 6)]:
            want = _torch_shape(nn.Conv3d.forward, m, torch.zeros((1, 1) + dhw))
            assert want is not None and m.out_dhw(dhw) == want, (k, s, dhw)
