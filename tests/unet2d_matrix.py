"""The 2-D U-Net / U-FNO option matrix: the case table and the builders shared by test_unet2d_matrix_host.py (CPU)
and test_gpu_unet2d_matrix.py (MI355X).  Importing this file needs neither a GPU nor libnps_hip.so; `build_module`
imports the project's modules when it is called.

A case is (hidden, ch_mults, n_blocks, padding_mode, norm, use1x1, n_cond, (H, W), B), attention off everywhere.
The reference of every row is oracle.functional.unet_modern / ufno evaluated in float64 on the float64 copy of the
state_dict and inputs (tests/test_oracle_golden.py pins that oracle to the reference project's goldens in fp32,
test_unet2d_matrix_host.py in fp64), forward and autograd backward with a seeded gy.

What default initialisation hides is randomised: every GroupNorm weight is uniform in [0.5, 1.5], every GroupNorm
bias uniform in [-0.3, 0.3] and every conv bias uniform in +-[0.05, 0.25] (gamma = 1, beta = 0 cannot catch a
misindexed affine).  Inputs are uniform in [-1, 1] from a seeded torch.Generator.
"""
import itertools
import math
from typing import NamedTuple, Optional, Tuple

import torch

from oracle import functional as Fo


class Case(NamedTuple):
    hidden: int
    ch_mults: Tuple[int, ...]
    n_blocks: int
    padding_mode: str
    norm: bool
    use1x1: bool
    n_cond: int
    hw: Tuple[int, int]
    B: int


class Row(NamedTuple):
    id: str
    kind: str   # "unet" | "ufno" (hidden_blocks 2, fno_modes 4)
    case: Case


UFNO_BLOCKS, UFNO_MODES = 2, 4


def row_id(kind, hidden, ch_mults, n_blocks, pm, norm, use1x1, n_cond, size, B):
    """The id scheme of a matrix row, shared with tests/unet3d_matrix.py (`size` = the grid, any rank)."""
    return (f"{kind}-h{hidden}-m{''.join(map(str, ch_mults))}-b{n_blocks}-{pm[:4]}-{'gn' if norm else 'nogn'}-"
            f"{'k1' if use1x1 else 'k3'}-c{n_cond}-{'x'.join(map(str, size))}-B{B}")


def _row(kind, hidden, ch_mults, n_blocks, pm, norm, use1x1, n_cond, hw, B):
    c = Case(hidden, tuple(ch_mults), n_blocks, pm, norm, use1x1, n_cond, tuple(hw), B)
    return Row(row_id(kind, *c), kind, c)


def _core_rows():
    """padding_mode x norm x use1x1 x n_cond {0, 4} at hidden 16, ch_mults [1, 2], one block per level, B 2 on the
    (21, 18) grid: the odd H (21 -> 11 -> 22 under 'ones'; every circular conv is a valid conv) puts every skip, vb
    and the output at non-zero crop offsets.  Four rows repeat at (24, 20): both paddings, both
    n_cond values, both norm and both use1x1 settings once."""
    rows = [_row("unet", 16, (1, 2), 1, pm, norm, k1, nc, (21, 18), 2)
            for pm, norm, k1, nc in itertools.product(("ones", "circular"), (True, False), (True, False), (0, 4))]
    rows += [_row("unet", 16, (1, 2), 1, pm, norm, k1, nc, (24, 20), 2)
             for pm, norm, k1, nc in (("ones", True, True, 4), ("ones", False, False, 0),
                                      ("circular", True, False, 0), ("circular", False, True, 4))]
    return rows


def _route_rows():
    both = ("ones", "circular")
    rows = []
    # nothing aligned (C % 16 != 0 everywhere, vb C = 2: its Downsample is the generic stride-2 conv); a second
    # block per level; B 3
    rows += [_row("unet", 8, (1, 2), 2, pm, True, True, 2, (21, 18), 3) for pm in both]
    # C % 4 == 0 but the skip starts at channel 24 / 48, off a 16-channel boundary: frame_pack with pad4
    rows += [_row("unet", 24, (1, 2), 1, pm, True, True, 4, (21, 18), 2) for pm in both]
    # C % 4 != 0 everywhere (6, 12, 7, 13, 25 channels)
    rows += [_row("unet", 6, (2, 1), 1, "ones", False, False, 1, (13, 10), 2)]
    # all three sources aligned (16 / 32 + 16-channel vb): vb's Downsample reads the space-to-depth view; three
    # levels.  The circular row needs (40, 36): at 24 x 20 the third level's valid convs run out of pixels.  Its
    # level-1 DownBlock is ResidualBlock(16 + 16, 32): an identity shortcut that adds cat(h, vb) itself
    rows += [_row("unet", 16, (1, 2, 2), 1, "ones", True, True, 16, (13, 10), 2),
             _row("unet", 16, (1, 2, 2), 1, "circular", True, True, 16, (40, 36), 2)]
    # a second block per level; identity shortcuts at mult 1 when n_cond = 0
    rows += [_row("unet", 32, (2, 1), 2, pm, True, True, nc, (21, 18), 2) for pm in both for nc in (0, 4)]
    # Cout 96 and 192: the wide 192-channel tile, the 1x1 shortcut at the fused-1x1 limit Cout = 192
    rows += [_row("unet", 48, (2, 2), 1, "ones", True, True, 4, (13, 10), 2),
             _row("unet", 48, (2, 2), 1, "circular", True, True, 4, (24, 20), 2),
             _row("unet", 48, (2, 2), 1, "ones", True, False, 4, (13, 10), 2)]
    # Cout 256 > 192, Cin up to 516
    rows += [_row("unet", 64, (2, 2), 1, "ones", True, True, 4, (13, 10), 1),
             _row("unet", 64, (2, 2), 1, "circular", True, True, 4, (24, 20), 1)]
    # a single-resolution circular U-Net with a valid 3x3 final conv: the final output is smaller than the input
    # and crop_Nd zero-pads it (the zero border)
    rows += [ZERO_BORDER_ROW]
    # tiles that are almost all padding
    rows += [_row("unet", 16, (1, 1), 1, "ones", False, True, 4, (5, 4), 2),
             _row("unet", 16, (1, 1), 1, "ones", False, True, 4, (3, 3), 1)]
    # C1's structure at its real width
    rows += [_row("unet", 32, (2, 2, 1, 2), 2, "circular", True, True, 4, (64, 64), 1)]
    return rows


ZERO_BORDER_ROW = _row("unet", 16, (1,), 1, "circular", True, False, 4, (12, 10), 2)
UFNO_BORDER_ROW = _row("ufno", 16, (1,), 1, "circular", True, False, 4, (12, 10), 2)


def _ufno_rows():
    """hidden_blocks 2, fno_modes 4 (4 <= H and 4 <= W // 2 + 1 on every grid here: the HIP spectral path accepts
    all of them, none was moved)."""
    return [_row("ufno", 16, (1, 1), 1, "circular", True, True, 4, (24, 20), 2),
            _row("ufno", 16, (1, 1), 1, "circular", True, True, 0, (24, 20), 2),
            _row("ufno", 32, (1, 2), 1, "ones", True, False, 4, (21, 18), 2),
            UFNO_BORDER_ROW]


ROWS = _core_rows() + _route_rows() + _ufno_rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def find(kind="unet", **want):
    """The one row of that kind whose case fields equal `want`."""
    hits = [r for r in ROWS if r.kind == kind and all(getattr(r.case, k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, [r.id for r in hits])
    return hits[0]


def oracle_cfg(row: Row) -> dict:
    c = row.case
    cfg = dict(hidden_features=c.hidden, ch_mults=c.ch_mults, n_blocks=c.n_blocks, padding_mode=c.padding_mode,
               norm=c.norm, use1x1=c.use1x1, n_cond=c.n_cond)
    if row.kind == "ufno":
        cfg.update(hidden_blocks=UFNO_BLOCKS, fno_modes=UFNO_MODES, fno_kernel_size=1, fno_conv_mode="single")
    return cfg


def oracle_fn(row: Row):
    return Fo.ufno if row.kind == "ufno" else Fo.unet_modern


def _seed(row: Row) -> int:
    return 1000 + [r.id for r in ROWS].index(row.id)


# ------------------------------------------------------------------------------------------- parameters
def _is_norm_key(k):
    return k.rsplit(".", 2)[-2].startswith("norm")


def randomise_(sd: dict, g: torch.Generator):
    """In place on a state_dict's tensors: GroupNorm weight ~ U[0.5, 1.5], GroupNorm bias ~ U[-0.3, 0.3], every
    conv bias of magnitude U[0.05, 0.25] with a random sign (never zero)."""
    with torch.no_grad():
        for k in sorted(sd):
            t = sd[k]
            if _is_norm_key(k):
                u = torch.rand(t.shape, generator=g)
                t.copy_(0.5 + u if k.endswith(".weight") else 0.6 * u - 0.3)
            elif k.endswith(".bias"):
                u = torch.rand(t.shape, generator=g)
                s = torch.randint(0, 2, t.shape, generator=g) * 2 - 1
                t.copy_(s * (0.05 + 0.2 * u))
    return sd


def _conv_entries(sd, key, cout, cin, k, g, transposed=False, nd=2):
    bound = 1.0 / math.sqrt((cout if transposed else cin) * k ** nd)  # nn.ConvNd's default: U(+-1/sqrt(fan_in))
    shape = ((cin, cout) if transposed else (cout, cin)) + (k,) * nd
    sd[key + ".weight"] = (torch.rand(shape, generator=g) * 2 - 1) * bound
    sd[key + ".bias"] = torch.zeros(cout)


def _res_entries(sd, p, cin, cout, norm, g, nd=2):
    if norm:
        for n, c in (("norm1", cin), ("norm2", cout)):
            sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"] = torch.ones(c), torch.zeros(c)
    _conv_entries(sd, p + ".conv1", cout, cin, 3, g, nd=nd)
    _conv_entries(sd, p + ".conv2", cout, cout, 3, g, nd=nd)
    if cin != cout:
        _conv_entries(sd, p + ".shortcut", cout, cin, 1, g, nd=nd)


def _unet_entries(sd, p, c, g, nd=2):
    """The state_dict keys and shapes of UNetModern (reference proc_unet_modern.py:91-152) from
    oracle.functional.unet_structure; `p` = key prefix with its trailing dot, `nd` = the convs' spatial rank (`c` is
    this file's Case or the 3-D matrix's: only the fields both have are read)."""
    down, _, up = Fo.unet_structure(c.hidden, c.ch_mults, c.n_blocks, c.n_cond)
    for i, m in enumerate(down):
        if m[0] == "down":
            _res_entries(sd, f"{p}down.{i}.res", m[1], m[2], c.norm, g, nd)
        else:
            _conv_entries(sd, f"{p}down.{i}.conv", m[1], m[1], 3, g, nd=nd)
            if c.n_cond > 0:
                _conv_entries(sd, f"{p}down.{i}.conv_variables_broadcast", c.n_cond, c.n_cond, 3, g, nd=nd)
    top = c.hidden * math.prod(c.ch_mults)
    _res_entries(sd, f"{p}middle.res1", top + c.n_cond, top, c.norm, g, nd)
    _res_entries(sd, f"{p}middle.res2", top, top, c.norm, g, nd)
    for i, m in enumerate(up):
        if m[0] == "up":  # UpBlock(cin, cout).res = ResidualBlock(cin + cout, cout): the skip has cout channels
            _res_entries(sd, f"{p}up.{i}.res", m[1] + m[2], m[2], c.norm, g, nd)
        else:
            _conv_entries(sd, f"{p}up.{i}.conv", m[1], m[1], 4, g, transposed=True, nd=nd)
    if c.norm:
        sd[p + "norm.weight"], sd[p + "norm.bias"] = torch.ones(c.hidden), torch.zeros(c.hidden)
    _conv_entries(sd, p + "final", c.hidden, c.hidden, 1 if c.use1x1 else 3, g, nd=nd)


def standin_state_dict(row: Row) -> dict:
    """A float32 state_dict with the module's keys and shapes and seeded stand-in weights (torch's default conv
    bounds, then randomise_): what the host tests run the oracle on, with no module and no shared library."""
    c = row.case
    g = torch.Generator().manual_seed(_seed(row))
    sd = {}
    if row.kind == "unet":
        _unet_entries(sd, "", c, g)
    else:
        cin, m = c.hidden + c.n_cond, UFNO_MODES
        for i in range(UFNO_BLOCKS):
            for w in ("weights1", "weights2"):  # SpectralConv2d: scale * rand(cfloat), scale = 1 / (cin * cout)
                sd[f"fno_layers.{i}.conv.{w}"] = torch.complex(
                    torch.rand(cin, c.hidden, m, m, generator=g), torch.rand(cin, c.hidden, m, m, generator=g)
                ) / (cin * c.hidden)
            _conv_entries(sd, f"fno_layers.{i}.w", c.hidden, cin, 1, g)
            _unet_entries(sd, f"unet_layers.{i}.", c, g)
    return randomise_(sd, g)


def build_module(row: Row):
    """The project's UNetModern / UFNO for the row (CPU, seeded), with randomise_ applied to its parameters."""
    from torch import nn
    from models.enc_proc_dec_components import UFNO, UNetModern
    c = row.case
    kw = dict(pde=None, num_spatial_dims=2, n_cond=c.n_cond, hidden_features=c.hidden, activation=nn.GELU(),
              norm=c.norm, ch_mults=list(c.ch_mults), is_attn=[False] * len(c.ch_mults), mid_attn=False,
              n_blocks=c.n_blocks, use1x1=c.use1x1, padding_mode=c.padding_mode)
    torch.manual_seed(_seed(row))
    if row.kind == "ufno":
        m = UFNO(hidden_blocks=UFNO_BLOCKS, fno_modes=UFNO_MODES, fno_kernel_size=1, fno_conv_mode="single", **kw)
    else:
        m = UNetModern(**kw)
    randomise_(dict(m.named_parameters()), torch.Generator().manual_seed(_seed(row)))
    return m


# ------------------------------------------------------------------------------------------- inputs / reference
def inputs(row: Row):
    """(h, vb or None, gy): float32, h and vb uniform in [-1, 1], gy standard normal, seeded per row."""
    return seeded_inputs(row.case, row.case.hw, 5000 + _seed(row))


def seeded_inputs(c, size, seed):
    """inputs() of a case on the grid `size` (any rank) from one seeded generator: h, vb, gy in that order."""
    g = torch.Generator().manual_seed(seed)
    h = torch.rand(c.B, c.hidden, *size, generator=g) * 2 - 1
    vb = torch.rand(c.B, c.n_cond, *size, generator=g) * 2 - 1 if c.n_cond > 0 else None
    gy = torch.randn(c.B, c.hidden, *size, generator=g)
    return h, vb, gy


class Ref(NamedTuple):
    y: torch.Tensor
    dh: Optional[torch.Tensor]
    dvb: Optional[torch.Tensor]
    grads: Optional[dict]


def _cast(t, dtype):
    if t is None:
        return None
    if t.is_complex():
        return t.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    return t.to(dtype)


def reference(row: Row, sd: dict, h, vb, gy=None, dtype=torch.float64) -> Ref:
    """The oracle on the `dtype` copy of sd and the inputs; with gy also dh, dvb and every parameter gradient."""
    return oracle_reference(oracle_fn(row), oracle_cfg(row), sd, h, vb, gy, dtype)


def oracle_reference(fn, cfg, sd: dict, h, vb, gy=None, dtype=torch.float64) -> Ref:
    """reference() for the oracle function `fn` and its cfg (tests/unet3d_matrix.py passes the 3-D ones)."""
    sd = {k: _cast(v.detach().cpu(), dtype).clone() for k, v in sd.items()}
    h, vb = _cast(h, dtype).clone(), _cast(vb, dtype)
    if gy is None:
        with torch.no_grad():
            return Ref(fn(sd, "", cfg, h, vb), None, None, None)
    for t in sd.values():
        t.requires_grad_(True)
    h.requires_grad_(True)
    if vb is not None:
        vb = vb.clone().requires_grad_(True)
    y = fn(sd, "", cfg, h, vb)
    y.backward(_cast(gy, dtype))
    return Ref(y.detach(), h.grad, vb.grad if vb is not None else None, {k: t.grad for k, t in sd.items()})

