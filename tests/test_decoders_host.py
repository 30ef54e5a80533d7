"""CPU checks of the grid decoders (dec_grid.py): the plain-torch restatement tests/decoders_ref.py against the
reference's recorded fp64 outputs and gradients (tests/golden/decoders_mod_*.pt) at 1e-12, the classes' state_dict
layout against the same fixtures, the size formulas, the host refusals of the decode descriptor (include/nps.h
nps_decode_t) and of the modules, and Swish on a CPU tensor."""
import ctypes
import glob
import os
import subprocess
import types

import pytest
import torch
from torch import nn

from conftest import GOLDEN, ROOT, load_golden, rel_l2
import decoders_ref as R

CASES = sorted(os.path.basename(p)[len("decoders_mod_"):-3] for p in glob.glob(os.path.join(GOLDEN, "decoders_mod_*.pt")))


def _build(g, dt=None):
    from models.enc_proc_dec_components import dec_grid
    extra = {} if g["cls"] in ("TimeConv", "LinearConv") else dict(activation=nn.GELU())
    m = getattr(dec_grid, g["cls"])(pde=types.SimpleNamespace(dt=g["dt"] if dt is None else dt), **g["kwargs"], **extra)
    if g["cls"] == "TimeConv":
        m.decoder[1].beta = g["beta"]
    return m


def test_fixture_list():
    assert len(CASES) == 16 and {load_golden(f"decoders_mod_{c}")["cls"] for c in CASES} == set(R.DECODERS)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(case):
    g = load_golden(f"decoders_mod_{case}")
    kw = dict(g["kwargs"], beta=g["beta"])
    y, gh, grads = R.reference_sd(lambda sd, h: R.decoder(g["cls"], sd, h, g["u"].double(), g["dt"], kw),
                                  g["state_dict"], g["h"], g["g"])
    errs = dict(y=rel_l2(y, g["y64"]), h=rel_l2(gh, g["gh64"]), **{k: rel_l2(grads[k], v) for k, v in g["grads64"].items()})
    assert set(grads) == set(g["grads64"])
    assert max(errs.values()) < 1e-12, errs


@pytest.mark.parametrize("case", CASES)
def test_state_dict_layout(case):
    """Same keys and shapes as the reference's module, which then loads strictly."""
    g = load_golden(f"decoders_mod_{case}")
    m = _build(g)
    sd = m.state_dict()
    assert list(sd) == list(g["state_dict"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in g["state_dict"].items()}
    m.load_state_dict(g["state_dict"], strict=True)
    for attr in ("pde", "num_spatial_dims", "time_window", "num_c", "dec_delta_mode", "dec_delta_dt"):
        assert hasattr(m, attr), attr
    assert all(callable(getattr(m, f)) for f in ("run", "run_ad", "forward"))


@pytest.mark.parametrize("tw", range(1, 27))
def test_size_formulas_yield_tw(tw):
    """TimeConvLinear's decoder_input_dim / kernel_size_a and TimeConv's stride / kernelsize give exactly tw outputs."""
    from models.enc_proc_dec_components import dec_grid
    pde = types.SimpleNamespace(dt=0.1)
    m = dec_grid.TimeConvLinear(pde=pde, num_c=2, num_spatial_dims=2, time_window=tw, hidden_features=8,
                                activation=nn.GELU())
    k = m.decoder.kernel_size[0]
    assert m.decoder_input_dim == R.timeconvlinear_dim(tw) and m.decoder.stride == (2,)
    assert m.pre_decoder.out_channels == 2 * m.decoder_input_dim
    assert (m.decoder_input_dim - k) // 2 + 1 == tw
    for hidden in (16, 32, 48, 128):
        if hidden // (tw + 9) == 0:
            with pytest.raises(AssertionError, match="stride 0"):
                dec_grid.TimeConv(pde=pde, num_c=2, num_spatial_dims=2, time_window=tw, hidden_features=hidden)
            continue
        t = dec_grid.TimeConv(pde=pde, num_c=2, num_spatial_dims=2, time_window=tw, hidden_features=hidden)
        s, k1 = t.decoder[0].stride[0], t.decoder[0].kernel_size[0]
        assert (s, k1) == R.timeconv_sizes(hidden, tw)
        L1 = (hidden - k1) // s + 1
        assert L1 - 10 + 1 == tw, (hidden, tw, s, k1)


def test_timeconv_sizes_of_the_gpu_cases():
    assert [R.timeconv_sizes(h, tw) for h, tw in ((16, 5), (32, 5), (48, 4), (128, 25))] == \
        [(1, 3), (2, 5), (3, 10), (3, 27)]


def test_swish_on_cpu():
    from models.common import Swish
    x = torch.linspace(-4, 4, 41, dtype=torch.float64)
    assert torch.equal(Swish()(x), x * torch.sigmoid(x))
    assert torch.equal(Swish(beta=0.5)(x), x * torch.sigmoid(0.5 * x))
    assert Swish()(x.float()).dtype == torch.float32


# ------------------------------------------------------------------ the descriptor
def _desc(**kw):
    import nps_hip
    d = nps_hip.DecodeArgs()
    d.x, d.out, d.u, d.dtcum = 0x1000, 0x2000, 0x3000, 0x4000
    d.w1 = d.b1 = d.w2 = d.b2 = 0x5000
    d.B, d.N = 2, 67
    for k, v in kw.items():
        setattr(d, k, v)
    CL = d.C0 * d.L0
    d.x_bs, d.x_ps, d.x_cs = CL * d.N, 1, d.N
    return d


def _refused(d, bwd=False):
    import nps_hip
    lib = nps_hip.lib
    rc = lib.nps_decode_bwd(ctypes.byref(d), 0x6000, 0x7000, None, None, None, None, None, None) if bwd else \
        lib.nps_decode_fwd(ctypes.byref(d), None)
    return rc, lib.nps_last_error().decode()


def test_descriptor_layout_matches_header():
    """ctypes mirror vs a C compile of the header (offsetof / sizeof), as test_cabi.py does for the other structs."""
    import nps_hip
    fields = [f for f, _ in nps_hip.DecodeArgs._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"nps.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(nps_decode_t));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(nps_decode_t, {f}));\n'
    prog += "return 0;}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(tmp, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(nps_hip.DecodeArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(nps_hip.DecodeArgs, f).offset == int(off), f
    assert len(fields) == len(out) - 1 == 31


@pytest.mark.parametrize("bwd", [False, True])
def test_descriptor_refuses_a_wrong_final_length(bwd):
    """The last stage must yield num_c x tw: the message names the sizes; no launch (there is no GPU here)."""
    # TimeConvLinear's sizes for tw = 5 (L0 = 12, k 3, stride 2 -> 5) with tw = 6 asked for
    rc, msg = _refused(_desc(nstage=1, C0=2, L0=12, C1=2, k1=3, s1=2, num_c=2, tw=6), bwd)
    assert rc < 0 and "2 channels x 5 positions" in msg and "tw=6" in msg, msg
    # two stages: 8 x 34 -> k2 = 10 -> 25, with num_c = 2 channels asked of a 3-channel stage
    rc, msg = _refused(_desc(nstage=2, C0=1, L0=128, C1=8, k1=27, s1=3, act=2, C2=3, k2=10, num_c=2, tw=25), bwd)
    assert rc < 0 and "3 channels x 25 positions" in msg and "num_c=2" in msg, msg
    # no stage: C0 * L0 must be num_c * tw
    rc, msg = _refused(_desc(nstage=0, C0=2, L0=5, num_c=2, tw=6), bwd)
    assert rc < 0 and "2*5" in msg and "2*6" in msg, msg
    # a kernel longer than the signal, a stride of 0, an unknown mode
    assert _refused(_desc(nstage=1, C0=1, L0=4, C1=1, k1=5, s1=1, num_c=1, tw=1), bwd)[0] < 0
    assert _refused(_desc(nstage=1, C0=1, L0=4, C1=1, k1=2, s1=0, num_c=1, tw=3), bwd)[0] < 0
    rc, msg = _refused(_desc(nstage=0, C0=2, L0=5, num_c=2, tw=5, delta_mode=3), bwd)
    assert rc < 0 and "delta_mode=3" in msg
    # per-pixel arrays beyond the LDS budget even at 8 pixels per work-group
    rc, msg = _refused(_desc(nstage=0, C0=1, L0=20000, num_c=1, tw=20000, delta_mode=2), bwd)
    assert rc < 0 and "LDS" in msg, msg


def test_workspace_size_of_the_backward():
    """At most 1024 rows of [w1 | b1 | w2 | b2]; one row per pixel group of 64 (32 when 64 pixels' arrays exceed the
    LDS budget) below that; 0 for a refused descriptor."""
    import nps_hip
    lib = nps_hip.lib
    d = _desc(nstage=2, C0=2, L0=15, C1=4, k1=3, s1=2, act=1, C2=2, k2=3, num_c=2, tw=5)
    nparams = 4 * 2 * 3 + 4 + 2 * 4 * 3 + 2
    assert lib.nps_decode_bwd_ws_floats(ctypes.byref(d)) == 2 * 2 * nparams          # N = 67: 2 groups per sample
    d.N = 1 << 20
    assert lib.nps_decode_bwd_ws_floats(ctypes.byref(d)) == 1024 * nparams
    big = _desc(nstage=2, C0=1, L0=128, C1=8, k1=27, s1=3, act=2, C2=3, k2=10, num_c=3, tw=25)  # TimeConv at the cfgs' sizes
    assert lib.nps_decode_bwd_ws_floats(ctypes.byref(big)) == 2 * 3 * (8 * 27 + 8 + 3 * 8 * 10 + 3)  # 32-pixel groups
    d.tw = 6
    assert lib.nps_decode_bwd_ws_floats(ctypes.byref(d)) == 0


def test_decode_chain_refuses_cpu_tensors():
    from nps_hip import ops
    spec = ops.DecodeSpec(planar=True, C0=2, L0=5, num_c=2, tw=5, delta_mode=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_chain(spec, torch.zeros(1, 10, 7), torch.zeros(1, 2, 5, 7))
    from models.enc_proc_dec_components.dec_grid import add_delta
    with pytest.raises(RuntimeError, match="MI355X"):
        add_delta(torch.zeros(1, 2, 5, 7), torch.zeros(1, 2, 5, 7), 0.1, 5, 1)
    with pytest.raises(ValueError, match="Unrecognized dec_delta_mode"):
        add_delta(torch.zeros(1, 2, 5, 7), torch.zeros(1, 2, 5, 7), 0.1, 5, 1, delta_mode="some")


@pytest.mark.parametrize("case", ["tcl_2d", "tc_h32", "tcd_all", "lc_k3_circ"])
def test_supported_decoders_reach_the_device_check(case):
    """The control of the refusal tests below: a decoder that has a path fails on CPU inputs at the device check."""
    g = load_golden(f"decoders_mod_{case}")
    m = _build(g)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        m(g["h"], g["u"])


def test_linearconv_3d_is_refused_before_any_launch():
    g = load_golden("decoders_mod_lc_3d")
    m = _build(g)
    m.load_state_dict(g["state_dict"])
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="LinearConv.*3-D"):
            m(g["h"], g["u"])
    with pytest.raises(NotImplementedError, match="LinearConv.*3-D"):
        m.run(torch.zeros(2, 12, 5, 4), g["u"])


def test_timeconvdense_non_gelu_is_refused_before_any_launch():
    from models.enc_proc_dec_components.dec_grid import TimeConvDense
    for mode in ("per_step", "all", "none"):
        m = TimeConvDense(pde=types.SimpleNamespace(dt=0.1), num_c=2, num_spatial_dims=2, time_window=5,
                          hidden_features=16, activation=nn.ReLU(), dec_delta_mode=mode)
        for grad in (False, True):
            with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="GELU"):
                m(torch.zeros(1, 16, 4, 4), torch.zeros(1, 2, 5, 4, 4))


def test_encprocdec_resolves_every_decoder():
    import models
    pde = types.SimpleNamespace(dt=0.1, n_cond_static=0, n_cond_spatial=0)
    for name, extra in (("TimeConvLinear", {}), ("TimeConv", {}), ("TimeConvDense", {}),
                        ("LinearConv", dict(dec_kernel_size=3, dec_padding_mode="circular"))):
        m = models.EncProcDec(pde=pde, encoder="enc_grid.ElementWise", processor="FNO", decoder=f"dec_grid.{name}",
                              num_c=1, num_spatial_dims=2, time_window=5, hidden_features=16, hidden_blocks=1,
                              fno_modes=2, activation=nn.GELU(), **extra)
        assert type(m.decoder).__name__ == name
