"""The 3-D U-Net / U-FNO option matrix: the case table and the builders shared by test_unet3d_matrix_host.py (CPU)
and test_gpu_unet3d_matrix.py (MI355X), the 3-D counterpart of tests/unet2d_matrix.py, whose dimension-free pieces
(randomise_, Ref, _cast, the row-id scheme, the stand-in state_dict entries, the seeded inputs and the oracle call) it
uses.  Importing this file needs neither a GPU nor libnps_hip.so; `build_module` imports the project's modules when it
is called.

A case is (hidden, ch_mults, n_blocks, norm, use1x1, n_cond, (D, H, W), B), attention off everywhere and
padding_mode "circular" throughout: the 3-D Upsample is defined for nothing else (oracle.functional.unet_modern3d
raises otherwise).  The reference of every row is oracle.functional.unet_modern3d / ufno3d evaluated in float64 on
the float64 copy of the state_dict and inputs (spectral weights complex128), forward and autograd backward with a
seeded gy.  Parameters and inputs are randomised exactly as in the 2-D matrix: GroupNorm weight U[0.5, 1.5], GroupNorm
bias U[-0.3, 0.3], conv biases of magnitude U[0.05, 0.25] with a random sign, inputs U[-1, 1], gy standard normal,
everything seeded per row.

Geometry (checked by test_unet3d_matrix_host.py).  Every circular conv is a valid conv.  A ResidualBlock keeps its
input extent (crop_Nd zero-pads its valid convs back), the Downsample is a valid stride-2 conv, n -> (n - 3) // 2 + 1,
and the lowest level needs 5 voxels per axis (the two valid 3x3x3 convs of a block shrink 5 to 1): one level needs
>= 5 per axis, two >= 11, three >= 23.  The Upsample gives 2 n + 6 (circular pad 1, then ConvTranspose3d(k 4, s 2)),
so the up path runs LARGER than the skips (5 -> 16 beside a skip of 11): every skip and vb is zero-padded into its
frame at a non-zero crop offset, and the output is cropped back.  The shapes are the smallest that reach each path.
"""
import itertools
import zlib
from typing import NamedTuple, Tuple

import torch

from oracle import functional as Fo
from unet2d_matrix import (Ref, _cast, _conv_entries, _unet_entries, oracle_reference,  # noqa: F401
                           randomise_, row_id, seeded_inputs)

PADDING_MODE = "circular"


class Case(NamedTuple):
    hidden: int
    ch_mults: Tuple[int, ...]
    n_blocks: int
    norm: bool
    use1x1: bool
    n_cond: int
    dhw: Tuple[int, int, int]
    B: int


class Row(NamedTuple):
    id: str
    kind: str   # "unet" | "ufno" (2 blocks, fno_modes (3, 4, 3)) | "c5" (one U-FNO block, bench.C5_UFNO_CFG's modes)
    case: Case


UFNO_BLOCKS, UFNO_MODES = 2, (3, 4, 3)


def _row(kind, hidden, ch_mults, n_blocks, norm, use1x1, n_cond, dhw, B):
    c = Case(hidden, tuple(ch_mults), n_blocks, norm, use1x1, n_cond, tuple(dhw), B)
    return Row(row_id(kind, hidden, c.ch_mults, n_blocks, PADDING_MODE, norm, use1x1, n_cond, c.dhw, B), kind, c)


G0 = (11, 12, 13)   # 11 -> 5, 12 -> 5, 13 -> 6; the up path at (16, 16, 18): crop offsets (3|2, 2, 3|2), both parities
G1 = (14, 12, 11)   # 14 -> 6, 12 -> 5, 11 -> 5; the up path at (18, 16, 16)
G2 = (11, 11, 12)   # the smallest two-level grid that still has an even axis


def _core_rows():
    """norm x use1x1 x n_cond {0, 4} at hidden 16, ch_mults (1, 2), one block per level, B 2 on (11, 12, 13): odd and
    even axes mix, so the skips, vb and the output sit at non-zero crop offsets of both parities.  Two rows repeat at
    (14, 12, 11): between them both norm settings, both use1x1 settings and both n_cond values."""
    rows = [_row("unet", 16, (1, 2), 1, norm, k1, nc, G0, 2)
            for norm, k1, nc in itertools.product((True, False), (True, False), (0, 4))]
    rows += [_row("unet", 16, (1, 2), 1, True, False, 0, G1, 2), _row("unet", 16, (1, 2), 1, False, True, 4, G1, 2)]
    return rows


def _c5_cfg():
    """bench.C5_UFNO_CFG (importing bench loads torch only).  Its own hidden_blocks (4) becomes 1: the blocks are
    copies of one structure, the other U-FNO rows chain two (a block's carried moments feed the next block's norm1),
    and one block of this width already takes the fp64 oracle 1.7 s forward and backward."""
    from bench import C5_UFNO_CFG
    return dict(C5_UFNO_CFG, hidden_blocks=1, fno_modes=tuple(C5_UFNO_CFG["fno_modes"]))


def _c5_row():
    """C5's structure (hidden 64, n_cond 4, ch_mults [1, 1], one block, GroupNorm, 1x1x1 final, modes (8, 12, 12)) at
    B 1 on the smallest grid it admits: two levels need 11 per axis, the modes need 8 <= D, 12 <= H and
    12 <= W // 2 + 1, i.e. W >= 22."""
    cfg = _c5_cfg()
    m1, m2, m3 = cfg["fno_modes"]
    dhw = (max(11, m1), max(11, m2), max(11, 2 * (m3 - 1)))
    return _row("c5", cfg["hidden_features"], cfg["ch_mults"], cfg["n_blocks"], cfg["norm"], cfg["use1x1"],
                cfg["n_cond"], dhw, 1)


ZERO_BORDER_ROW = _row("unet", 16, (1,), 1, True, False, 4, (6, 7, 9), 2)
UFNO_BORDER_ROW = _row("ufno", 16, (1,), 1, True, False, 4, (6, 7, 9), 2)
TINY_ROW = _row("unet", 16, (1,), 1, True, True, 4, (5, 5, 6), 1)
IDENT_CAT_ROW = _row("unet", 16, (1, 2), 1, True, True, 16, G0, 2)
IDENT_CAT_UFNO_ROW = _row("ufno", 16, (1, 2), 1, True, True, 16, G0, 2)
DEPTH_ROW = _row("unet", 16, (1, 1, 2), 1, True, True, 4, (23, 24, 25), 1)
WIDE192_ROW = _row("unet", 48, (2, 2), 1, True, True, 4, G2, 1)
WIDE256_ROW = _row("unet", 64, (2, 2), 1, True, True, 4, G2, 1)
C5_ROW = _c5_row()


def _route_rows():
    rows = []
    # channel alignment: nothing a multiple of 16 (8, 16 | 10, 18, 26, 34 channel frames, vb C = 2), two blocks, B 3
    rows += [_row("unet", 8, (1, 2), 2, True, True, 2, G0, 3)]
    # C % 4 == 0 but sources off a 16-channel boundary: frame_pack3d pads the 28- and 52-channel frames
    rows += [_row("unet", 24, (1, 2), 1, True, True, 4, G0, 2)]
    # C % 4 != 0 everywhere (6, 12 | 7, 13, 25 channels); hidden % 8 != 0 is no valid model with norm=True (the final
    # norm is GroupNorm(8, hidden)), so norm=False as in 2-D
    rows += [_row("unet", 6, (2, 1), 1, False, False, 1, G2, 2)]
    # identity shortcut on a concatenation: hidden 16 + n_cond 16, so the level-1 DownBlock is ResidualBlock(32, 32)
    # and its identity shortcut adds cat(h, vb) itself
    rows += [IDENT_CAT_ROW]
    # identity shortcut on a single source: hidden 32, (2, 1), two blocks per level, without and with conditioning
    rows += [_row("unet", 32, (2, 1), 2, True, True, nc, G0, 2) for nc in (0, 4)]
    # wide: Cout 192 (past c3d_1x1_eligible's 128), then Cout 256 with Cin up to 516, then C5's structure
    rows += [WIDE192_ROW, WIDE256_ROW]
    # depth: three levels, 23 -> 11 -> 5
    rows += [DEPTH_ROW]
    # a single level with a valid 3x3x3 final conv (crop_Nd zero-pads it: the zero border), and a single level at
    # (5, 5, 6): the blocks' valid convs shrink 5 to 1, the frames are almost all padding
    rows += [ZERO_BORDER_ROW, TINY_ROW]
    return rows


def _ufno_rows():
    """hidden_blocks 2, fno_modes (3, 4, 3), kernel 1, "single": (1, 1) with and without conditioning, the
    identity-on-concatenation configuration (the block output's carried moments then feed the next block's norm1),
    the single-level border geometry (tests/test_gpu_ufno3d.py::test_ufno3d_single_resolution_valid_final_conv_border
    keeps its own copy at hidden 8 / n_cond 2), and C5's structure.  The two (1, 1) rows sit on (14, 12, 11), not
    (11, 12, 13): two U-FNO blocks double the depth, and there the fp32 ORACLE is 1.0e-6 / 1.2e-6 from the fp64 one,
    over the host file's 1e-6 bound (0.6e-6 ... 1.2e-6 over six candidate grids; 6.8e-7 / 6.9e-7 on this one)."""
    return [_row("ufno", 16, (1, 1), 1, True, True, 4, G1, 2), _row("ufno", 16, (1, 1), 1, True, True, 0, G1, 2),
            IDENT_CAT_UFNO_ROW, UFNO_BORDER_ROW, C5_ROW]


ROWS = _core_rows() + _route_rows() + _ufno_rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}
# the rows whose inference form also runs on bf16 storage (test_gpu_unet3d_matrix.py): aligned hidden 16 with n_cond 4,
# C5's structure, one U-FNO, and the Cout-192 row (the only way past c3d_1x1_eligible's Cout <= 128 in bf16); and the
# two geometries bf16 storage refuses by design
BF16_ROWS = (ROWS[1], C5_ROW, _ufno_rows()[0], WIDE192_ROW)
BF16_REFUSED = {UFNO_BORDER_ROW.id: "a final conv smaller than its input under a fused addend",
                IDENT_CAT_ROW.id: "an identity shortcut on a concatenated input"}


def find(kind="unet", **want):
    """The one row of that kind whose case fields equal `want`."""
    hits = [r for r in ROWS if r.kind == kind and all(getattr(r.case, k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, [r.id for r in hits])
    return hits[0]


def is_ufno(row: Row) -> bool:
    return row.kind in ("ufno", "c5")


def ufno_modes(row: Row):
    return _c5_cfg()["fno_modes"] if row.kind == "c5" else UFNO_MODES


def ufno_blocks(row: Row) -> int:
    return _c5_cfg()["hidden_blocks"] if row.kind == "c5" else UFNO_BLOCKS


def level_extents(dhw, n_levels):
    """The grid at every level: the circular Downsample is a valid stride-2 conv, n -> (n - 3) // 2 + 1."""
    out = [tuple(dhw)]
    for _ in range(n_levels - 1):
        out.append(tuple((n - 3) // 2 + 1 for n in out[-1]))
    return out


def oracle_cfg(row: Row) -> dict:
    c = row.case
    cfg = dict(hidden_features=c.hidden, ch_mults=c.ch_mults, n_blocks=c.n_blocks, padding_mode=PADDING_MODE,
               norm=c.norm, use1x1=c.use1x1, n_cond=c.n_cond)
    if is_ufno(row):
        cfg.update(hidden_blocks=ufno_blocks(row), fno_modes=ufno_modes(row), fno_kernel_size=1, fno_conv_mode="single")
    return cfg


def oracle_fn(row: Row):
    return Fo.ufno3d if is_ufno(row) else Fo.unet_modern3d


def _seed(row: Row) -> int:
    """From the row's id, so that a row keeps its parameters and inputs when the table around it changes."""
    return 3000 + zlib.crc32(row.id.encode()) % 100000


def standin_state_dict(row: Row) -> dict:
    """A float32 state_dict with the module's keys and shapes and seeded stand-in weights (torch's default conv
    bounds, then randomise_): conv weights (Cout, Cin, k, k, k), transposed (Cin, Cout, 4, 4, 4), SpectralConv3d
    weights1..4 (Cin, Cout, m1, m2, m3) complex64."""
    c = row.case
    g = torch.Generator().manual_seed(_seed(row))
    sd = {}
    if not is_ufno(row):
        _unet_entries(sd, "", c, g, nd=3)
    else:
        cin, modes = c.hidden + c.n_cond, ufno_modes(row)
        for i in range(ufno_blocks(row)):
            for n in range(1, 5):  # SpectralConv3d: scale * rand(cfloat), scale = 1 / (cin * cout)
                sd[f"fno_layers.{i}.conv.weights{n}"] = torch.complex(
                    torch.rand(cin, c.hidden, *modes, generator=g), torch.rand(cin, c.hidden, *modes, generator=g)
                ) / (cin * c.hidden)
            _conv_entries(sd, f"fno_layers.{i}.w", c.hidden, cin, 1, g, nd=3)
            _unet_entries(sd, f"unet_layers.{i}.", c, g, nd=3)
    return randomise_(sd, g)


def build_module(row: Row):
    """The project's 3-D UNetModern / UFNO for the row (CPU, seeded), with randomise_ applied to its parameters."""
    from torch import nn
    from models.enc_proc_dec_components import UFNO, UNetModern
    c = row.case
    kw = dict(pde=None, num_spatial_dims=3, n_cond=c.n_cond, hidden_features=c.hidden, activation=nn.GELU(),
              norm=c.norm, ch_mults=list(c.ch_mults), is_attn=[False] * len(c.ch_mults), mid_attn=False,
              n_blocks=c.n_blocks, use1x1=c.use1x1, padding_mode=PADDING_MODE)
    torch.manual_seed(_seed(row))
    if is_ufno(row):
        m = UFNO(hidden_blocks=ufno_blocks(row), fno_modes=ufno_modes(row), fno_kernel_size=1, fno_conv_mode="single",
                 **kw)
    else:
        m = UNetModern(**kw)
    randomise_(dict(m.named_parameters()), torch.Generator().manual_seed(_seed(row)))
    return m


def inputs(row: Row):
    """(h, vb or None, gy): float32 (B, C, D, H, W), h and vb uniform in [-1, 1], gy standard normal, seeded per row."""
    return seeded_inputs(row.case, row.case.dhw, 5000 + _seed(row))


def reference(row: Row, sd: dict, h, vb, gy=None, dtype=torch.float64) -> Ref:
    """The 3-D oracle on the `dtype` copy of sd and the inputs; with gy also dh, dvb and every parameter gradient."""
    return oracle_reference(oracle_fn(row), oracle_cfg(row), sd, h, vb, gy, dtype)
