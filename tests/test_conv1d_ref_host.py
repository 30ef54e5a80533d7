"""No GPU: the fp64 restatement of the 1-D conv entries (tests/conv1d_ref.py) against torch's own F.conv1d /
F.conv_transpose1d in float64 and torch.autograd, the ctypes mirrors of the new structs against include/nps.h, the
host-side argument checks of the entries, and the refusal of CPU / non-fp32 tensors before any launch."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn.functional as F

import conv1d_ref as R
from conftest import ROOT

GEOS = [(1, 1, (0, 0)), (3, 1, (1, 1)), (3, 2, (1, 1)), (4, 2, (1, 1)), (2, 1, (1, 0)), (4, 1, (1, 2))]


def _cl(t):
    """(B, C, L) <-> (B, L, C)"""
    return t.transpose(1, 2).contiguous()


@pytest.mark.parametrize("K,s,pad", GEOS)
@pytest.mark.parametrize("L", [5, 8, 13])
def test_forward_is_f_conv1d(K, s, pad, L):
    x, w, b = R.rand((2, L, 5), 1).double(), R.rand((4, 5, K), 2).double(), R.rand((4,), 3).double()
    want = F.conv1d(F.pad(_cl(x), pad), w, b, stride=s)
    got = R.conv1d_fwd([(x, 0)], L, w, b, stride=s, pad=pad)
    torch.testing.assert_close(_cl(got), want, rtol=1e-12, atol=1e-12)


def test_forward_frame_is_cat_of_cropped_sources():
    """three sources: one at -1 (cropped on the left), one shorter than the frame placed at 2, one covering it"""
    L = 9
    a, b, c = R.rand((2, L, 3), 1), R.rand((2, L + 1, 2), 2), R.rand((2, 4, 4), 3)
    fr = R.frame([(a, 0), (b, -1), (c, 2)], L)
    want = torch.cat((a.double(), b[:, 1:1 + L].double(), F.pad(c.double(), (0, 0, 2, L - 6))), 2)
    assert torch.equal(fr, want)
    w, bias = R.rand((6, 9, 3), 4), R.rand((6,), 5)
    got = R.conv1d_fwd([(a, 0), (b, -1), (c, 2)], L, w, bias, pad=(1, 1))
    torch.testing.assert_close(_cl(got), F.conv1d(_cl(want), w.double(), bias.double(), padding=1), rtol=1e-12,
                               atol=1e-12)


def test_forward_epilogue_addend_gelu_accumulate_offset():
    L = 7
    x, w, b = R.rand((2, L, 3), 1), R.rand((4, 3, 3), 2), R.rand((4,), 3)
    y = F.conv1d(_cl(x).double(), w.double(), b.double(), padding=1)           # (2, 4, 7)
    out0, add = R.rand((2, 10, 6), 4), R.rand((2, 10, 6), 5)
    got = R.conv1d_fwd([(x, 0)], L, w, b, pad=(1, 1), out=out0, out_off=2, accumulate=True, addend=add, act=1)
    want = out0.double().clone()
    want[:, 2:9, :4] += F.gelu(_cl(y) + add[:, 2:9, :4].double())
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # a negative offset drops the rows that fall outside out
    got = R.conv1d_fwd([(x, 0)], L, w, b, pad=(1, 1), out=torch.zeros(2, 4, 4), out_off=-2)
    torch.testing.assert_close(got, _cl(y)[:, 2:6], rtol=1e-12, atol=1e-12)
    assert R.written_rows(7, 4, 1, -2) == [0, 1, 2, 3]


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("L", [1, 6, 7])
def test_two_phases_are_conv_transpose1d(p, L):
    x, w, b = R.rand((2, L, 3), 1).double(), R.rand((3, 5, 4), 2).double(), R.rand((5,), 3).double()
    want = F.conv_transpose1d(_cl(x), w, b, stride=2, padding=p)
    torch.testing.assert_close(_cl(R.conv_transpose1d(x, w, b, p)), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("K,s,pad", GEOS)
@pytest.mark.parametrize("L", [6, 9])
def test_gradients_are_autograd_of_f_conv1d(K, s, pad, L):
    x = R.rand((2, L, 5), 1).double().requires_grad_(True)
    w = R.rand((4, 5, K), 2).double().requires_grad_(True)
    y = F.conv1d(F.pad(x.transpose(1, 2), pad), w, None, stride=s)
    gy = R.rand(tuple(y.shape), 3).double()
    (y * gy).sum().backward()
    dy = _cl(gy)
    torch.testing.assert_close(R.conv1d_dx(dy, w.detach(), L, s, pad), x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv1d_dw(dy, x.detach(), K, s, pad), w.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("p", [0, 1])
def test_transposed_gradients_are_the_swapped_entries(p):
    """dx of a k4/s2 transposed conv = the K = 4 / stride-2 / pad-p conv of dy with the weight read as (out = Cin,
    in = Cout, k); dw = the weight-gradient entry with a = x and x = dy."""
    L = 7
    x = R.rand((2, L, 3), 1).double().requires_grad_(True)
    w = R.rand((3, 5, 4), 2).double().requires_grad_(True)
    y = F.conv_transpose1d(x.transpose(1, 2), w, None, stride=2, padding=p)
    gy = R.rand(tuple(y.shape), 3).double()
    (y * gy).sum().backward()
    dy = _cl(gy)
    torch.testing.assert_close(R.conv1d_fwd([(dy, 0)], dy.shape[1], w.detach(), None, stride=2, pad=(p, p)), x.grad,
                               rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv1d_dw(x.detach(), dy, 4, 2, (p, p)), w.grad, rtol=1e-12, atol=1e-12)


def test_derived_weights_give_the_input_gradients():
    """The weights nps_hip.ops derives for the input gradients, applied through the restated forward entry: stride 1
    (flipped taps, channels swapped) and stride 2 (the two phases of the transposed conv with the conv's own weight)."""
    from nps_hip import ops
    L = 9
    x, w = R.rand((2, L, 5), 1), R.rand((4, 5, 3), 2)
    dy = R.rand((2, L, 4), 3)
    got = R.conv1d_fwd([(dy, 0)], L, ops.conv1d_dgrad_weight(w), None, pad=(1, 1))
    torch.testing.assert_close(got, R.conv1d_dx(dy, w, L, 1, (1, 1)), rtol=1e-12, atol=1e-12)
    Ly = R.out_len(L, 3, 2, (1, 1))
    dy = R.rand((2, Ly, 4), 4)
    dx = torch.zeros(2, L, 5)
    for r, wr in enumerate(ops.conv_transpose1d_phase_weights(w)):
        dx = R.conv1d_fwd([(dy, 0)], Ly, wr, None, pad=(1, 1), out=dx, out_os=2, out_off=r - 1)
    torch.testing.assert_close(dx, R.conv1d_dx(dy, w, L, 2, (1, 1)), rtol=1e-12, atol=1e-12)
    for r in (0, 1):
        wt = R.rand((3, 5, 4), 5)
        assert torch.equal(ops.conv_transpose1d_phase_weights(wt)[r], R.phase_weight(wt, r))


# ------------------------------------------------------------------ C ABI
@pytest.mark.parametrize("cstruct,pyname", [("nps_conv1d_t", "Conv1dArgs"), ("nps_wgrad1d_t", "Wgrad1dArgs"),
                                            ("nps_src1_t", "Src1")])
def test_struct_layout_matches_header(cstruct, pyname):
    """ctypes mirror vs a C compile of the header (offsetof / sizeof)."""
    import nps_hip
    Args = getattr(nps_hip, pyname)
    fields = [f for f, _ in Args._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"nps.h\"\nint main(){\n"
    prog += f'printf("%zu\\n", sizeof({cstruct}));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof({cstruct}, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(Args)
    for f, off in zip(fields, out[1:]):
        assert getattr(Args, f).offset == int(off), f


def _fwd_args(**kw):
    import nps_hip
    a = nps_hip.Conv1dArgs()
    a.nsrc = 1
    a.src[0].ptr, a.src[0].C, a.src[0].L = 0x1000, 18, 33
    a.B, a.Lc, a.Cin = 2, 33, 18
    a.K, a.stride, a.pad_l, a.pad_r, a.Lout = 3, 1, 1, 1, 33
    a.wpack, a.Cout = 0x2000, 16
    a.out, a.out_C, a.out_L, a.out_os = 0x3000, 16, 33, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [(dict(K=5), "K 5"), (dict(stride=3), "stride 3"), (dict(Lout=34), "Lout 34"),
                                     (dict(Cin=20), "Cin is 20"), (dict(out_C=8), "out_C 8"), (dict(out_os=3), "out_os 3"),
                                     (dict(nsrc=4), "nsrc 4"), (dict(act=2), "act 2"), (dict(wpack=0x2004), "wpack")])
def test_forward_entry_checks_its_arguments_on_the_host(kw, word):
    import nps_hip
    assert nps_hip.lib.nps_conv1d_fwd(ctypes.byref(_fwd_args(**kw)), None) < 0
    assert word in nps_hip.lib.nps_last_error().decode()


def test_wgrad_entry_checks_and_fixed_split_schedule():
    """The workspace is splits x K x padded M x padded N floats, a function of the shape alone: asking twice gives
    the same schedule; bad arguments give 0 / < 0 with a message."""
    import nps_hip
    lib = nps_hip.lib
    p = nps_hip.Wgrad1dArgs()
    p.a, p.B, p.La, p.M = 0x1000, 16, 2048, 128
    p.x, p.Lx, p.N = 0x2000, 2048, 130
    p.K, p.stride, p.pad_l, p.pad_r = 3, 1, 1, 1
    n = lib.nps_conv1d_wgrad_ws_floats(ctypes.byref(p))
    assert n == lib.nps_conv1d_wgrad_ws_floats(ctypes.byref(p)) and n > 0
    assert n % (3 * 128 * 192) == 0 and 1 <= n // (3 * 128 * 192) <= 64
    p.La = 2047
    assert lib.nps_conv1d_wgrad_ws_floats(ctypes.byref(p)) == 0 and b"a's length 2047" in lib.nps_last_error()
    p.La, p.K = 2048, 5
    assert lib.nps_conv1d_wgrad(ctypes.byref(p), None) < 0 and b"K 5" in lib.nps_last_error()
    p.K = 3
    assert lib.nps_conv1d_wgrad(ctypes.byref(p), None) < 0 and b"null tensor" in lib.nps_last_error()
    assert lib.nps_conv1d_packed_floats(40, 34, 3) == 3 * 48 * 64 and lib.nps_conv1d_packed_floats(4, 4, 5) == 0


def test_activation_only_prologue_of_a_1x1_conv_is_not_fused():
    """A norm=False U-Net with use1x1=True ends in a 1x1 conv with a GELU prologue and no GroupNorm.  The split-fp16
    1x1 kernel's fused prologue reads the GroupNorm affine for its input range, so the host routes that conv through
    nps_frame_pack (ops.conv2d asks nps_conv2d_x3_prologue_ok) and nps_conv2d_fwd refuses the fused form."""
    import nps_hip
    from nps_hip import ops
    lib = nps_hip.lib
    assert lib.nps_conv2d_x3_prologue_ok(1, 1, 16, 0, 1) == 0
    assert lib.nps_conv2d_x3_prologue_ok(1, 1, 16, 1, 1) == 1 and lib.nps_conv2d_x3_prologue_ok(1, 1, 32, 8, 0) == 1
    assert lib.nps_conv2d_x3_prologue_ok(3, 3, 16, 0, 1) == 1 and lib.nps_conv2d_x3_prologue_ok(3, 3, 16, 1, 1) == 1
    a = nps_hip.Conv2dArgs()
    a.nsrc = 1
    a.src[0].ptr, a.src[0].C, a.src[0].H, a.src[0].W = 0x1000, 16, 1, 20
    a.B, a.Hin, a.Win, a.Cin = 2, 1, 20, 16
    a.KH = a.KW = a.stride = a.dil = 1
    a.Hout, a.Wout, a.Cout = 1, 20, 16
    a.out, a.wpack, a.out_C, a.out_H, a.out_W, a.out_os = 0x2000, 0x3000, 16, 1, 20, 1
    a.precision, a.pre_act = ops.PREC_X3F16, 1
    lib.nps_conv2d_plan(ctypes.byref(a))
    assert lib.nps_conv2d_fwd(ctypes.byref(a), None) < 0


# ------------------------------------------------------------------ refusals
def test_ops_refuse_cpu_and_non_fp32_tensors():
    from nps_hip import ops
    from nps_hip import autograd as ad
    x, w = torch.zeros(1, 8, 4), torch.zeros(4, 4, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.pack_conv1d_weight(w)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.conv1d([ops.Src1(x)], 8, w, None, 4, 3, pad=(1, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.conv1d_wgrad(x, x, 3, pad=(1, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        ad.Conv1dFn.apply((3, 1, 1, 1), x.view(1, 1, 8, 4), w, None)
    with pytest.raises(RuntimeError, match="MI355X"):
        ad.ConvTranspose1dFn.apply(1, x.view(1, 1, 8, 4), torch.zeros(4, 4, 4), None)


def test_the_1d_unet_marks_its_own_pointwise_convs_exact():
    """The 1-D U-Net's 1x1 shortcuts and use1x1 final conv take the exact-fp32 Conv1d kernels (Conv1d.exact, set by
    the constructors: no parameter, not in the state_dict); the FNO layer's `w` keeps the 2-D route, and so does every
    2-D module."""
    from models.common import Conv1d
    from models.enc_proc_dec_components import UFNO, UNetModern
    m = UFNO(pde=None, num_spatial_dims=1, n_cond=2, hidden_features=16, hidden_blocks=1, fno_modes=3,
             padding_mode="ones")
    point = {k: c for k, c in m.named_modules() if isinstance(c, Conv1d) and c.pointwise()}
    assert any(".shortcut" in k for k in point) and any(k.endswith(".final") for k in point)
    for k, c in point.items():
        assert c.exact == (k.startswith("unet_layers.")), k
        assert c._taps() == c.exact
    assert all(c._taps() for c in m.modules() if isinstance(c, Conv1d) and not c.pointwise())
    assert not any("exact" in k for k in m.state_dict())
    m2 = UNetModern(pde=None, num_spatial_dims=2, n_cond=2, hidden_features=8, ch_mults=[1, 2], n_blocks=1, use1x1=True)
    assert not any(getattr(c, "exact", False) for c in m2.modules())
    circ = Conv1d(4, 4, 1, padding_mode="circular")
    circ.exact = True
    assert not circ._taps()  # (only zero-padded convs take the Conv1d kernels)


def test_modules_refuse_cpu_tensors_and_keep_their_parameters():
    from torch import nn
    from models.common import Conv1d, ConvTranspose1d, get_upconv_with_right_spatial_dim
    from nps_hip import ops
    torch.manual_seed(3)
    up = get_upconv_with_right_spatial_dim(1, 6, 6, kernel_size=4, stride=2, padding=1)
    torch.manual_seed(3)
    ref = nn.ConvTranspose1d(6, 6, kernel_size=4, stride=2, padding=1)
    assert isinstance(up, ConvTranspose1d) and isinstance(up, nn.ConvTranspose1d)
    assert list(up.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(up.state_dict().values(), ref.state_dict().values()))
    c = Conv1d(6, 4, 3, stride=2, padding=1)
    assert c.geometry1d() == (3, 2, 1, 1) and c.out_hw(1, 13) == (1, 7)
    assert Conv1d(6, 4, 4, padding="same").geometry1d() == (4, 1, 1, 2)
    assert Conv1d(6, 4, 2, padding="valid").out_hw(1, 9) == (1, 8)
    x = torch.zeros(2, 1, 13, 6)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            with pytest.raises(RuntimeError, match="MI355X"):
                c.run_ad(x) if grad else c.run([ops.Src(x)], (1, 13))
            with pytest.raises(RuntimeError, match="MI355X"):
                up(torch.zeros(2, 6, 13))
    for bad in (Conv1d(6, 4, 5, padding=2), Conv1d(6, 4, 3, dilation=2), Conv1d(6, 6, 3, groups=2),
                Conv1d(6, 4, 3, padding=3)):  # (stride-1 padding beyond K - 1: run_ad has no input gradient for it)
        with pytest.raises(NotImplementedError):
            bad.run([ops.Src(x)], (1, 13))
