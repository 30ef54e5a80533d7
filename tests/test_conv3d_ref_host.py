"""No GPU: the fp64 restatement of the 3-D conv forward (tests/conv3d_ref.py) against torch's own modules, the
elementwise bound against a CPU fp32 conv of every plain row, and the route every row of the tables reaches
(nps_conv3d_route: the launcher's own dispatch, host arithmetic only)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv3d_ref as R

F32, BF16 = torch.float32, torch.bfloat16


def _module(c, cls, **kw):
    inp = R.inputs(c.name)
    m = cls(c.Cin, c.Cout, 4 if c.transposed else c.K, **kw).double()
    with torch.no_grad():
        m.weight.copy_(inp.w)
        m.bias.copy_(inp.bias)
    return m, inp


def test_reference_is_circular_conv3d():
    c = R.BY_NAME["s_k3s1_circ1"]
    m, inp = _module(c, nn.Conv3d, padding=1, padding_mode="circular")
    torch.testing.assert_close(R.refs(c.name, F32), m(inp.xs[0].double()), rtol=1e-12, atol=1e-12)


def test_reference_is_zero_padded_stride2_conv3d():
    c = R.BY_NAME["s_k3s2_zpad1"]
    m, inp = _module(c, nn.Conv3d, padding=1, stride=2)
    torch.testing.assert_close(R.refs(c.name, F32), m(inp.xs[0].double()), rtol=1e-12, atol=1e-12)


def test_reference_is_circular_pad_then_conv_transpose3d():
    """the 3-D Upsample: circular pad 1 on every axis, then ConvTranspose3d(k = 4, s = 2, p = 0)"""
    c = R.BY_NAME["s_k2_transposed"]
    m, inp = _module(c, nn.ConvTranspose3d, stride=2)
    want = m(F.pad(inp.xs[0].double(), (1,) * 6, mode="circular"))
    assert want.shape == R.refs(c.name, F32).shape == (2, 68, 10, 18, 70)
    torch.testing.assert_close(R.refs(c.name, F32), want, rtol=1e-12, atol=1e-12)


def _crop_nd(x, off, dhw):
    """crop_Nd of a source into the frame: F.pad with the offsets (negative pads crop)"""
    pads = []
    for o, m, n in reversed(list(zip(off, x.shape[2:], dhw))):
        pads += [o, n - (o + m)]
    return F.pad(x, pads)


def test_reference_is_group_norm_gelu_on_a_cropped_three_source_frame():
    c = R.BY_NAME["g_k1_853_gn2_gelu"]
    inp = R.inputs(c.name)
    fr = torch.cat([_crop_nd(x.double(), s[4:7], c.dhw) for x, s in zip(inp.xs, c.srcs)], 1)
    assert float((fr[:, 8:] == 0).double().mean()) > 0.05     # uncovered voxels: normalised, not skipped
    n = F.gelu(F.group_norm(fr, 2, inp.gamma.double(), inp.beta.double(), eps=1e-5))
    want = F.conv3d(n, inp.w.double(), inp.bias.double())
    got = R.refs(c.name, F32)
    assert got.shape[1] == 10
    torch.testing.assert_close(got[:, :6], want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[:, 6:], inp.prefill.double()[:, 6:], rtol=0, atol=0)


def test_prologue_comes_before_the_extension():
    """the wrapped halo holds normalised values, the zero padding stays zero (beta != 0 makes act(GN(0)) visible)"""
    c = R.BY_NAME["g_k3s1_853_gn2_gelu"]
    inp = R.inputs(c.name)
    fr = torch.cat([_crop_nd(x.double(), s[4:7], c.dhw) for x, s in zip(inp.xs, c.srcs)], 1)
    n = F.gelu(F.group_norm(fr, 2, inp.gamma.double(), inp.beta.double(), eps=1e-5))
    assert float(n[fr == 0].abs().min()) > 1e-3
    ext = F.pad(F.pad(n, (1,) * 6, mode="circular"), (1,) * 6)
    want = F.conv3d(ext, inp.w.double(), inp.bias.double())
    torch.testing.assert_close(R.refs(c.name, F32)[:, :70], want, rtol=1e-12, atol=1e-12)


def test_epilogue_placement_and_accumulate():
    c = R.BY_NAME["e_f32_vec4_off_pos_larger"]
    inp = R.inputs(c.name)
    y = F.conv3d(inp.xs[0].double(), inp.w.double(), inp.bias.double())
    want = inp.prefill.double().clone()
    want[:, :, 1:1 + y.shape[2], 2:2 + y.shape[3], 3:3 + y.shape[4]] += y
    torch.testing.assert_close(R.refs(c.name, F32), want, rtol=1e-12, atol=1e-12)
    c = R.BY_NAME["e_f32_vec4_os2"]
    inp = R.inputs(c.name)
    y = F.conv3d(inp.xs[0].double(), inp.w.double(), inp.bias.double())
    got = R.refs(c.name, F32)
    torch.testing.assert_close(got[:, :, 1::2, 0::2, 1::2], y, rtol=1e-12, atol=1e-12)
    m = R.touched_mask(c)
    assert int(m.sum()) == y.numel() and torch.equal(got[~m], inp.prefill.double()[~m])
    c = R.BY_NAME["e_f32_vec4_off_neg_crop"]
    inp = R.inputs(c.name)
    y = F.conv3d(inp.xs[0].double(), inp.w.double(), inp.bias.double())[:, :, 1:, 2:, 3:][:, :, :1, :6, :30]
    torch.testing.assert_close(R.refs(c.name, F32), y + inp.addend.double(), rtol=1e-12, atol=1e-12)


PLAIN = [(n, dt) for n, dt in R.CONV_PARAMS if R.BY_NAME[n].plain]


@pytest.mark.parametrize("name,dt", PLAIN)
def test_bound_holds_for_a_cpu_fp32_conv(name, dt):
    """A correct fp32 conv of the row's operands lies inside the elementwise bound; rounded to bf16 it lies inside
    the bf16 bound."""
    c, dtype = R.BY_NAME[name], R.DTYPES[dt]
    ref = R.window(c, R.refs(name, dtype))
    y = R.window(c, R.reference(c, dtype, compute=torch.float32))
    if dtype == BF16:
        y = y.to(BF16)
    ratio = ((y.double() - ref).abs() / R.bound(c, dtype)).max().item()
    print(f"{name} {dt}: largest error / bound of a CPU fp32 conv {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bound_sees_a_dropped_tap(dt):
    """One tap of one input channel dropped leaves the bound at more than half of the outputs."""
    c, dtype = R.BY_NAME["s_k3s1_valid_rem"], R.DTYPES[dt]   # (a valid conv: the dropped tap never reads padding)
    inp = R.inputs(c.name)
    w = R._rt(inp.w, dtype).clone()
    w[:, 0, 0, 0, 0] = 0
    bad = F.conv3d(R._rt(inp.xs[0], dtype), w, inp.bias.double())
    out = (bad - R.refs(c.name, dtype)).abs() > R.bound(c, dtype)
    assert out.double().mean().item() > 0.5


@pytest.mark.parametrize("name,dt", R.CONV_PARAMS)
def test_row_reaches_the_route_it_names(name, dt):
    c = R.BY_NAME[name]
    assert R.route_of(R.launch_args(c, R.DTYPES[dt])) == c.route(dt)


def test_rows_cover_every_route():
    """The union of the rows is every instantiation nps_conv3d_fwd can launch without an environment knob (the four
    knob-selected ones: conv3d_ref.ALL_ROUTES' comment)."""
    reached = {R.route_of(R.launch_args(R.BY_NAME[n], R.DTYPES[dt])) for n, dt in R.CONV_PARAMS}
    assert reached == set(R.ALL_ROUTES), reached ^ set(R.ALL_ROUTES)
    assert len(R.ALL_ROUTES) == 28
    # the GENERAL K > 1 routes exist only with ops.CONV3D_PACK off: the same rows packed run the SIMPLE kernels
    for n, dt in R.CONV_PARAMS:
        c = R.BY_NAME[n]
        if not c.pack:
            assert "GENERAL" in c.route(dt)
            assert "SIMPLE" in R.route_of(R.launch_args(c._replace(pack=True), R.DTYPES[dt]))


def test_three_source_1x1x1_runs_the_generic_kernel():
    """c3d_1x1_eligible refuses three sources (tests/test_gpu_conv3d.py::test_conv3d_1x1x1_bf16_streaming's 132-channel
    frame): conv3d_kernel at four waves per SIMD, not conv3d_1x1_kernel<*,9,*>."""
    v = (5, 9, 37)
    c = R.Case("three", (), 2, ((64,) + v + (0, 0, 0), (64, 7, 7, 37, -1, 1, 0), (4, 3, 9, 37, 1, 0, 0)), v, 64, 1)
    assert R.route_of(R.launch_args(c, BF16)) == R.R("bf16", 1, 1, False, "REG_O4")
    two = c._replace(srcs=((128,) + v + (0, 0, 0), (4, 3, 9, 37, 1, 0, 0)))
    assert R.route_of(R.launch_args(two, BF16)) == R.R1(2, 9, False)


def test_route_query_checks_its_arguments():
    import ctypes
    import nps_hip
    a = R.launch_args(R.BY_NAME["s_k3s1_zpad1"], F32)
    small = ctypes.create_string_buffer(8)
    assert nps_hip.lib.nps_conv3d_route(ctypes.byref(a), small, len(small)) < 0
    a.Dout += 1    # (nps_conv3d_fwd's own argument checks come first)
    with pytest.raises(RuntimeError, match="output extent"):
        R.route_of(a)
    assert nps_hip.lib.nps_conv3d_1x1_set_grid(0) == 0


def test_geometry_of_the_rows():
    """What the tables promise: B = 2, Dout >= 2, a second row tile and a second 32-column tile with tails, more than
    8 work-groups; each kernel family has a row whose work-group count is no multiple of 8."""
    rem = set()
    for c in R.CONV_ROWS:
        if "1x1" in c.name:
            nvox = c.dhw[0] * c.dhw[1] * c.dhw[2]
            assert c.B == 2 and nvox % 32 != 0
            continue
        th = R.GEO[(c.K, c.stride)]
        Do, Ho, Wo = c.conv_dhw
        assert c.B == 2 and Do >= 2 and Ho % th == 1 and Ho > th and 33 <= Wo <= 40, c.name
        wgs = c.B * Do * -(-Ho // th) * -(-Wo // 32)
        assert wgs > 8
        if wgs % 8:
            rem.add((c.K, c.stride))
    assert rem == set(R.GEO)


@pytest.mark.parametrize("Cout,Cin,K,transposed", R.PACK_CASES)
def test_pack_reference_layout(Cout, Cin, K, transposed):
    """pack_weight_reference against the index formula of include/nps.h, element by element on a sample"""
    g = torch.Generator().manual_seed(Cout)
    w = torch.randn((Cin, Cout, 4, 4, 4) if transposed else (Cout, Cin, K, K, K), generator=g)
    p = R.pack_weight_reference(w, K, transposed)
    ntile, nchunk = -(-Cout // 64), -(-Cin // 16)
    assert p.numel() == (8 if transposed else 1) * ntile * K * nchunk * K * K * 64 * 16
    for i in torch.randint(0, p.numel(), (400,), generator=g).tolist():
        r, k = divmod(i, 16)
        r, col = divmod(r, 64)
        r, kw = divmod(r, K)
        r, kh = divmod(r, K)
        r, chunk = divmod(r, nchunk)
        r, kd = divmod(r, K)
        z, tile = divmod(r, ntile)
        co, ci = tile * 64 + col, chunk * 16 + k
        if co >= Cout or ci >= Cin:
            want = 0.0
        elif transposed:
            want = w[ci, co, (z >> 2) + 2 * (1 - kd), ((z >> 1) & 1) + 2 * (1 - kh), (z & 1) + 2 * (1 - kw)].item()
        else:
            want = w[co, ci, kd, kh, kw].item()
        assert p[i].item() == want, i
