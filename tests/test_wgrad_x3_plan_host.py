"""CPU checks of the split-fp16 weight gradient's split-K schedule (csrc/wgrad_x3.hip): the launcher's own plan
(nps_conv2d_wgrad_x3_plan: argument checks, kernel choice, wx_split — host arithmetic, dummy pointers, nothing
launches) under the kernels' decode of blockIdx.x (tests/wgrad_x3_plan.py).  A wrong tile range or decode would drop
or double-count pixel tiles; here every (tile, split) must appear once and every tile's splits must partition the
pixel tiles, over a few thousand geometries on both sides of the 256 / 512-work-group threshold."""
import ctypes
import random

import pytest

import wgrad_x3_plan as wp

CHANNELS = (4, 64, 68, 132, 196, 388)


# ---------------------------------------------------------------- refusals
def _refused(p):
    """(the plan query refuses, the launch refuses) — the launch with dummy range tags / workspace and a NULL
    stream: its host checks come first, so a refused geometry launches nothing."""
    import nps_hip
    out = (ctypes.c_int * 8)()
    rc_plan = nps_hip.lib.nps_conv2d_wgrad_x3_plan(ctypes.byref(p), out)
    rc_launch = nps_hip.lib.nps_conv2d_wgrad_x3(ctypes.byref(p), 0x4000, 0x5000, 0x6000, None)
    return rc_plan < 0, rc_launch < 0


def _set(**kw):
    def f(p):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


REFUSALS = [
    ("M % 4", _set(M=66), "multiples of 4"), ("N % 4", _set(N=34), "multiples of 4"),
    ("M, N % 4", _set(M=30, N=22), "multiples of 4"),
    ("k 0", _set(KH=0, KW=0), "unsupported"), ("k 4", _set(KH=4, KW=4), "unsupported"),
    ("k 5", _set(KH=5, KW=5), "unsupported"), ("KH != KW", _set(KH=3, KW=1), "unsupported"),
    ("dil 2", _set(dil=2), "unsupported"), ("dil 0", _set(dil=0), "unsupported"),
    ("circ < 0", _set(circ=-1), "unsupported"),
    ("a NULL", _set(a=None), "bad shape"), ("x NULL", _set(x=None), "bad shape"), ("g NULL", _set(g=None), "bad shape"),
    ("B 0", _set(B=0), "bad shape"), ("Wa 0", _set(Wa=0), "bad shape"), ("N 0", _set(N=0), "bad shape"),
    ("a off 16 B", _set(a=0x1004), "multiples of 4"), ("x off 16 B", _set(x=0x2008), "multiples of 4"),
]


@pytest.mark.parametrize("name,tweak,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refuses_where_the_launch_refuses(name, tweak, word):
    import nps_hip
    p = wp.args(2, 64, 36, 3, 1, 0, 20, 24)
    assert wp.query(p) is not None
    tweak(p)
    assert _refused(p) == (True, True), name
    assert word in nps_hip.lib.nps_last_error().decode()


def test_plan_refuses_null_arguments():
    import nps_hip
    lib = nps_hip.lib
    out = (ctypes.c_int * 8)()
    assert lib.nps_conv2d_wgrad_x3_plan(None, out) < 0
    assert lib.nps_conv2d_wgrad_x3(None, 0x4000, 0x5000, 0x6000, None) < 0
    p = wp.args(2, 64, 36, 3, 1, 0, 20, 24)
    assert lib.nps_conv2d_wgrad_x3_plan(ctypes.byref(p), None) < 0
    # the launch alone needs range tags and a workspace
    assert lib.nps_conv2d_wgrad_x3(ctypes.byref(p), None, 0x5000, 0x6000, None) < 0
    assert lib.nps_conv2d_wgrad_x3(ctypes.byref(p), 0x4000, None, 0x6000, None) < 0
    assert lib.nps_conv2d_wgrad_x3(ctypes.byref(p), 0x4000, 0x5000, None, None) < 0
    assert lib.nps_conv2d_wgrad_x3_plan(ctypes.byref(p), out) == 0


# ---------------------------------------------------------------- sweep
def _geometries():
    """(B, M, N, k, pad, circ, Ha, Wa): every k x (M, N) x B with a dozen extents from 1..90 each — small ones
    (splits of 1-3 tiles) as often as large ones — under plain, padded and circular variants; the threshold shapes
    (B = 2: 250 x 400 = 200 000 pixels exactly, 250 x 401 just over) for every k and (M, N); REGIMES' rows."""
    rng = random.Random(20240607)
    geo = []
    for k in (1, 2, 3):
        for M in CHANNELS:
            for N in CHANNELS:
                for B in (1, 2, 3):
                    for i in range(12):
                        hi = 12 if i % 3 == 0 else 90
                        Ha, Wa = rng.randint(1, hi), rng.randint(1, 90)
                        pad, circ = ((0, 0), (1, 0), (0, 1))[rng.randrange(3)]
                        if min(Ha, Wa) + k - 1 - 2 * pad - 2 * circ < 1:
                            pad = circ = 0
                        geo.append((B, M, N, k, pad, circ, Ha, Wa))
                for Wa in (400, 401):
                    geo.append((2, M, N, k, 0, 0, 250, Wa))
                    geo.append((2, M, N, k, 1, 0, 250, Wa))
    return geo + [case for case, _ in wp.REGIMES]


def _want_kernel(B, M, N, k, pad, circ, Ha, Wa):
    if k == 1 and pad == 0 and circ == 0:  # (equal extents follow: Hx = Ha + k - 1 - 2 pad - 2 circ)
        return wp.WIDE1
    if k == 2 and M > 64 and N > 64:
        return wp.WIDE2
    return wp.X3


def _check_schedule(pl, geo):
    """The kernels' decode over the whole grid: every (tile, split) once; each tile's splits partition the pixel
    tiles; under remap the tiles of one split are consecutive work-groups of one XCD."""
    where = {}
    for l in range(pl.grid):
        ts = wp.decode(pl, l)
        assert ts not in where, (geo, pl, l, ts)
        where[ts] = l
    assert set(where) == {(t, s) for t in range(pl.base) for s in range(pl.splits)}, (geo, pl)
    # (the ranges do not depend on the tile, and every tile has every split: one walk serves all tiles)
    nxt = 0
    for s in range(pl.splits):
        t0, t1 = wp.owned(pl, s)
        if t0 >= t1:
            assert pl.remap, (geo, pl, s)  # without remap every split owns a tile
            continue
        assert t0 == nxt and t1 - t0 <= pl.per, (geo, pl, s)
        nxt = t1
    assert nxt == pl.ntiles, (geo, pl)
    if pl.remap:
        for s in range(pl.splits):
            ls = [where[(t, s)] for t in range(pl.base)]
            assert len({l % 8 for l in ls}) == 1, (geo, pl, s)
            assert [l >> 3 for l in ls] == list(range(ls[0] >> 3, (ls[0] >> 3) + pl.base)), (geo, pl, s)


def test_schedule_sweep():
    geos = _geometries()
    assert len(geos) > 3000
    seen = {"remap": 0, "plain": 0, "empty": 0, "ragged": 0, "short": 0, "g512": 0, "g256_full": 0,
            wp.X3: 0, wp.WIDE1: 0, wp.WIDE2: 0}
    for geo in geos:
        B, M, N, k, pad, circ, Ha, Wa = geo
        pl = wp.plan(*geo)
        assert pl is not None, geo
        assert pl.kernel == _want_kernel(*geo), (geo, pl)
        rows = {wp.X3: 64, wp.WIDE1: 192, wp.WIDE2: 128}[pl.kernel]
        assert pl.n_nt == -(-N // rows) and pl.base == -(-M // rows) * pl.n_nt, (geo, pl)
        if pl.kernel == wp.WIDE1:
            ntiles = -(-B * Ha * Wa // 32)
        else:
            th = 2 if pl.kernel == wp.WIDE2 else 4
            ntiles = B * -(-Ha // th) * -(-Wa // 16)
        assert pl.ntiles == ntiles, (geo, pl)
        assert pl.splits >= 1 and pl.per >= 1
        if pl.remap:
            assert pl.splits % 8 == 0 and pl.grid == pl.base * pl.splits, (geo, pl)
        else:
            assert pl.grid == pl.base * pl.splits, (geo, pl)
            assert (pl.splits - 1) * pl.per < pl.ntiles, (geo, pl)  # every split owns at least one tile
        big = B * Ha * Wa > wp.PIXELS_512
        assert pl.grid <= (512 if big else 256), (geo, pl)
        assert pl.per * pl.splits >= pl.ntiles, (geo, pl)
        _check_schedule(pl, geo)
        owning, last = wp.last_owning(pl)
        seen["remap" if pl.remap else "plain"] += 1
        seen["empty"] += owning < pl.splits
        seen["ragged"] += last < pl.per
        seen["short"] += last <= 3
        seen["g512"] += pl.grid > 256
        seen["g256_full"] += (not big) and pl.grid == 256
        seen[pl.kernel] += 1
    assert all(v >= 20 for v in seen.values()), seen  # the sweep meets every regime, not one side of it


@pytest.mark.parametrize("k,M,N,grid", [(3, 68, 68, (256, 512)), (1, 196, 196, (256, 512)),
                                        (2, 132, 132, (256, 512)), (2, 64, 132, (240, 504))])
def test_grid_doubles_past_200000_pixels(k, M, N, grid):
    """B = 2, 250 x 400 is the last shape on the 256-work-group grid, 250 x 401 the first on the 512 one
    (2 x 64 x 132 has base 3: 85 -> 80 and 170 -> 168 splits)."""
    at, over = wp.plan(2, M, N, k, 0, 0, 250, 400), wp.plan(2, M, N, k, 0, 0, 250, 401)
    assert (at.grid, over.grid) == grid, (at, over)


@pytest.mark.parametrize("case", [(2, 8, 12, 3, 1, 0, 7, 9), (2, 12, 8, 3, 0, 1, 6, 5), (1, 8, 8, 2, 1, 0, 5, 6),
                                  (2, 8, 4, 2, 0, 1, 4, 7), (3, 4, 8, 1, 0, 0, 5, 3), (1, 8, 8, 1, 1, 0, 6, 6)])
def test_matmul_reference_is_the_conv_weight_gradient(case):
    """ref_wgrad (the GPU schedule tests' fp64 reference, k * k matmuls over shifted slices of the extended NHWC
    input) against torch.nn.grad.conv2d_weight — the reference of test_wgrad_x3_vs_fp64 — in fp64."""
    import torch
    import torch.nn.functional as F
    B, M, N, k, pad, circ, Ha, Wa = case
    Hx, Wx = Ha + k - 1 - 2 * pad - 2 * circ, Wa + k - 1 - 2 * pad - 2 * circ
    torch.manual_seed(3)
    a = torch.randn(B, M, Ha, Wa, dtype=torch.float64)
    x = torch.randn(B, N, Hx, Wx, dtype=torch.float64)
    xe = F.pad(x, (circ,) * 4, mode="circular") if circ else x
    want = torch.nn.grad.conv2d_weight(F.pad(xe, (pad,) * 4), (M, N, k, k), a)
    got = wp.ref_wgrad(a.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous(), k, pad, circ)
    assert (got - want).abs().max() < 1e-12


@pytest.mark.parametrize("case,times", [((1, 68, 68, 3, 1, 0, 75, 40), 0), ((1, 68, 68, 3, 1, 0, 75, 40), 2),
                                        ((1, 196, 196, 1, 0, 0, 57, 32), 0), ((1, 132, 132, 2, 0, 0, 38, 40), 2)])
def test_a_lost_or_doubled_tile_is_far_above_the_bars(case, times):
    """What the GPU tests' bars can see, on the CPU in fp64: the last pixel tile of a 57-tile case (the tile its
    1-tile last split owns) counted 0 or 2 times moves G's rel-L2 to ~ sqrt(1 / 57) and the bias row's to ~ 1e-2
    — three and four orders above the 1e-5 and 1e-6 bars of tests/test_gpu_wgrad_schedule.py."""
    import torch
    B, M, N, k, pad, circ, Ha, Wa = case
    pl = wp.plan(*case)
    assert pl.ntiles == 57 and wp.last_owning(pl) == (8, 1)
    torch.manual_seed(1)
    a = torch.randn(B, Ha, Wa, M, dtype=torch.float64) + 0.1
    x = torch.randn(B, Ha + k - 1 - 2 * pad, Wa + k - 1 - 2 * pad, N, dtype=torch.float64)
    ref, ref_db = wp.ref_wgrad(a, x, k, pad, circ), a.sum((0, 1, 2))
    bad = a.clone()
    if pl.kernel == wp.WIDE1:  # the last 32 pixels of the flat range
        bad.view(-1, M)[56 * 32:] *= times
    else:                      # the last th x 16-pixel tile: the bottom rows' right-most columns
        th = 2 if pl.kernel == wp.WIDE2 else 4
        ty, tx = -(-Ha // th) - 1, -(-Wa // 16) - 1
        bad[:, ty * th:, tx * 16:] *= times
    e = (wp.ref_wgrad(bad, x, k, pad, circ) - ref).norm() / ref.norm()
    edb = (bad.sum((0, 1, 2)) - ref_db).norm() / ref_db.norm()
    assert e > 1e-2 and edb > 1e-3, (e, edb)


@pytest.mark.parametrize("case,want", wp.REGIMES, ids=[str(c) for c, _ in wp.REGIMES])
def test_regime_table_matches_the_plan(case, want):
    """Each GPU case of tests/test_gpu_wgrad_schedule.py still runs the regime it was chosen for."""
    pl = wp.plan(*case)
    assert pl is not None and wp.regime(pl) == want, (case, pl)
    _check_schedule(pl, case)
