"""CPU checks of the 3-D conv backward: the nps_wgrad3d_t / Wgrad3dArgs layout against a C compile of the header,
nps_conv3d_wgrad's host refusals (nothing launches), and the weight derivations of the input gradients
(nps_hip.ops.conv3d_dgrad_weight / conv3d_s2_dgrad_weight / conv_transpose3d_dgrad_weight — torch ops on the
parameter before packing) against torch autograd in fp64."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


def test_wgrad3d_struct_layout_matches_header():
    """ctypes mirror vs a C compile of the header (offsetof / sizeof), as test_cabi.py does for the other structs."""
    import nps_hip
    Args = nps_hip.Wgrad3dArgs
    fields = [f for f, _ in Args._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"nps.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(nps_wgrad3d_t));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(nps_wgrad3d_t, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(Args)
    assert len(out) == 1 + len(fields) == 17
    for f, off in zip(fields, out[1:]):
        assert getattr(Args, f).offset == int(off), f


def _args(K=3, stride=1, circ=0, zpad=0, a=(5, 6, 7), x=(7, 8, 9)):
    import nps_hip
    p = nps_hip.Wgrad3dArgs()
    p.a, p.B, (p.Da, p.Ha, p.Wa), p.M = 0x1000, 2, a, 24
    p.x, (p.Dx, p.Hx, p.Wx), p.N = 0x2000, x, 20
    p.K, p.stride, p.circ, p.zpad, p.g = K, stride, circ, zpad, 0x3000
    return p


@pytest.mark.parametrize("kw,word", [(dict(K=5), "K 5"), (dict(K=0), "K 0"), (dict(stride=3), "stride 3"),
                                     (dict(stride=0), "stride 0"),
                                     (dict(a=(5, 6, 8)), "extent"),            # W: 9 - 3 + 1 = 7, not 8
                                     (dict(a=(4, 6, 7)), "extent"),            # D
                                     (dict(zpad=1), "extent"),                 # padded x: a would be 7x8x9
                                     (dict(stride=2, a=(3, 3, 5)), "extent"),  # stride 2: (3, 3, 4)
                                     (dict(K=4, stride=2, circ=1, a=(3, 4, 5)), "extent")])  # (3, 4, 4)
def test_wgrad3d_host_refusals(kw, word):
    """K outside 1..4, stride outside 1..2 and an a extent that is not the conv's output over the extended x are
    refused before any launch (dummy pointers, NULL stream, no GPU): rc < 0 and a message that names the cause."""
    import nps_hip
    lib = nps_hip.lib
    p = _args(**kw)
    assert lib.nps_conv3d_wgrad(ctypes.byref(p), None) < 0
    assert word in lib.nps_last_error().decode()
    assert lib.nps_conv3d_wgrad_splits(ctypes.byref(p)) < 0


@pytest.mark.parametrize("kw", [dict(), dict(zpad=1, a=(7, 8, 9)), dict(circ=1, a=(7, 8, 9)),
                                dict(stride=2, a=(3, 3, 4)), dict(stride=2, zpad=1, a=(4, 4, 5)),
                                dict(K=4, stride=2, circ=1, a=(3, 4, 4)), dict(K=2, a=(6, 7, 8)),
                                dict(K=1, a=(7, 8, 9))])
def test_wgrad3d_plan_accepts_matching_extents(kw):
    """The same host checks accept the matching geometries (the plan entry point launches nothing)."""
    import nps_hip
    assert nps_hip.lib.nps_conv3d_wgrad_splits(ctypes.byref(_args(**kw))) >= 1


def test_wgrad3d_plan_splits_the_reduction():
    """The forward test's shape (B = 2, Cin = 68, Cout = 48, 9x20x40, K = 3 valid): 2 * 7 * ceil(18/4) * ceil(38/16)
    = 210 voxel tiles over 1 x 2 channel tiles x 3 kd planes -> 8 tiles per work-group, 27 work-groups per
    reduction."""
    import nps_hip
    p = _args(a=(7, 18, 38), x=(9, 20, 40))
    p.M, p.N = 48, 68
    assert nps_hip.lib.nps_conv3d_wgrad_splits(ctypes.byref(p)) == 27


# ---------------------------------------------------------------- weight derivations (fp64, CPU)
def _autograd_dx(fwd, x, gy):
    x = x.clone().requires_grad_(True)
    y = fwd(x)
    assert y.shape == gy.shape
    (y * gy).sum().backward()
    return x.grad


@pytest.mark.parametrize("K,mode,p", [(3, "zeros", 0), (3, "zeros", 1), (3, "circular", 1), (2, "zeros", 0),
                                      (3, "zeros", 2)])
def test_stride1_dgrad_weight(K, mode, p):
    """dx = conv3d(dy extended by K - 1 - p zeros per side — circularly by p for circular 'same' —,
    conv3d_dgrad_weight(w)): the three stride-1 geometries of the U-Net (valid, zero padding 1, circular padding 1)
    and the bounds of the rule (K = 2; zero padding K - 1)."""
    from nps_hip import ops
    torch.manual_seed(0)
    x = torch.randn(2, 3, 5, 6, 7, dtype=torch.float64)
    w = torch.randn(4, 3, K, K, K, dtype=torch.float64)

    def fwd(t):
        if mode == "circular":
            return F.conv3d(F.pad(t, (p,) * 6, mode="circular"), w)
        return F.conv3d(t, w, padding=p)
    gy = torch.randn_like(fwd(x))
    wd = ops.conv3d_dgrad_weight(w)
    assert wd.shape == (3, 4, K, K, K) and wd.is_contiguous()
    if mode == "circular":
        dx = F.conv3d(F.pad(gy, (p,) * 6, mode="circular"), wd)
    else:
        dx = F.conv3d(F.pad(gy, (K - 1 - p,) * 6), wd)
    ref = _autograd_dx(fwd, x, gy)
    assert dx.shape == ref.shape and (dx - ref).abs().max() < 1e-12


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("dhw", [(6, 7, 9), (5, 8, 6)])
def test_stride2_dgrad_weight(p, dhw):
    """The stride-2 Downsample's dx = the k4/s2 transposed conv of dy with conv3d_s2_dgrad_weight(w) (the k3 weight
    zero-padded to k4), shifted by -p and cropped to x — every voxel of x lies inside that output, and those no
    output reads come out as exact zeros (6 with p = 0: depth index 5)."""
    from nps_hip import ops
    torch.manual_seed(1)
    x = torch.randn(2, 3, *dhw, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, 3, dtype=torch.float64)

    def fwd(t):
        return F.conv3d(t, w, stride=2, padding=p)
    gy = torch.randn_like(fwd(x))
    wt = ops.conv3d_s2_dgrad_weight(w)
    assert wt.shape == (4, 3, 4, 4, 4)
    full = F.conv_transpose3d(gy, wt, stride=2)
    assert all(full.shape[2 + i] - p >= dhw[i] for i in range(3))
    dx = full[:, :, p:p + dhw[0], p:p + dhw[1], p:p + dhw[2]]
    ref = _autograd_dx(fwd, x, gy)
    assert (dx - ref).abs().max() < 1e-12
    if p == 0 and dhw[0] == 6:
        assert (dx[:, :, 5] == 0).all() and (ref[:, :, 5] == 0).all()


def _s2d3(t):
    """NCDHW space-to-depth by 2: channel ((rd*2 + rh)*2 + rw)*C + c = t[c, 2 dq + rd, 2 hq + rh, 2 wq + rw]."""
    B, C, D, H, W = t.shape
    return (t.reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 3, 5, 7, 1, 2, 4, 6)
            .reshape(B, 8 * C, D // 2, H // 2, W // 2))


def test_conv_transpose_dgrad_weight():
    """The Upsample's dx: K = 2 conv of space-to-depth(dy) with conv_transpose3d_dgrad_weight(w), then the fold of
    the circular border."""
    from nps_hip import ops
    torch.manual_seed(2)
    x = torch.randn(2, 3, 2, 4, 5, dtype=torch.float64)
    w = torch.randn(3, 5, 4, 4, 4, dtype=torch.float64)

    def fwd(t):
        return F.conv_transpose3d(F.pad(t, (1,) * 6, mode="circular"), w, stride=2)
    gy = torch.randn_like(fwd(x))
    wd = ops.conv_transpose3d_dgrad_weight(w)
    assert wd.shape == (3, 40, 2, 2, 2)
    dxp = F.conv3d(_s2d3(gy), wd)                       # gradient of the padded input (4, 6, 7)
    assert dxp.shape == (2, 3, 4, 6, 7)
    xp = x.clone().requires_grad_(True)
    F.pad(xp, (1,) * 6, mode="circular").backward(dxp)  # torch's fold
    ref = _autograd_dx(fwd, x, gy)
    assert (xp.grad - ref).abs().max() < 1e-12
