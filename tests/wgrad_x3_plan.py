"""Host model of the split-fp16 weight gradient's split-K schedule (csrc/wgrad_x3.hip).

The launcher's plan comes from the library itself (nps_conv2d_wgrad_x3_plan: host arithmetic, nothing launches);
`decode` is the kernels' own map from blockIdx.x to (tile, split) — the same lines open wgrad_x3_kernel,
wgrad1_wide_kernel and wgrad2_wide_kernel — and `owned` the pixel-tile range [t_begin, t_end) a split runs its
software pipeline over (empty: the work-group returns at once).
"""
import ctypes
from collections import namedtuple

Plan = namedtuple("Plan", "kernel ntiles base n_nt splits per remap grid")
X3, WIDE1, WIDE2 = 0, 1, 2  # Plan.kernel: wgrad_x3_kernel<KH, KW>, wgrad1_wide_kernel, wgrad2_wide_kernel
PIXELS_512 = 200000         # B * Ha * Wa above this runs a 512-work-group grid, 256 up to it (wx_wgs)


# The schedule's edge regimes, one geometry each: (B, M, N, k, pad, circ, Ha, Wa) -> the regime it was chosen for,
# (kernel, ntiles, base, owning splits, splits, tiles per split, remap, tiles of the last owning split).  Splits
# that own 1, 2 or 3 tiles run the pipelines' prologue / epilogue paths (wgrad_x3_kernel fetches two tiles ahead,
# the wide kernels one); `owning < splits` are grids whose trailing work-groups return at once.  The host test
# holds every row to the plan query and tests/test_gpu_wgrad_schedule.py runs it against fp64: after a retune of
# wx_split / wx_wgs pick a new geometry for the regime with this model, do not drop the row.
REGIMES = [
    # wgrad_x3_kernel<3, 3>
    ((1, 64, 64, 3, 1, 0, 4, 16), (X3, 1, 1, 1, 1, 1, 0, 1)),          # one tile
    ((1, 68, 36, 3, 1, 0, 5, 13), (X3, 2, 2, 1, 1, 2, 0, 2)),          # two tiles
    ((1, 36, 68, 3, 0, 1, 9, 16), (X3, 3, 2, 1, 1, 3, 0, 3)),          # three tiles, circular
    ((1, 68, 68, 3, 1, 0, 50, 70), (X3, 65, 4, 9, 9, 8, 0, 1)),        # plain order, last split 1 tile
    ((1, 68, 68, 3, 1, 0, 75, 40), (X3, 57, 4, 8, 8, 8, 1, 1)),        # remap 8, last split 1 tile
    ((2, 68, 36, 3, 0, 1, 66, 60), (X3, 136, 2, 16, 16, 9, 1, 1)),     # 17 -> 16 rounding, last 1, circular
    ((1, 68, 68, 3, 1, 0, 170, 40), (X3, 129, 4, 15, 16, 9, 1, 3)),    # remap with an empty 16th split
    # wgrad_x3_kernel<2, 2> (M <= 64)
    ((1, 64, 96, 2, 0, 0, 3, 9), (X3, 1, 2, 1, 1, 1, 0, 1)),
    ((1, 64, 132, 2, 1, 0, 50, 70), (X3, 65, 3, 9, 9, 8, 0, 1)),
    ((1, 36, 132, 2, 0, 0, 75, 40), (X3, 57, 3, 8, 8, 8, 1, 1)),
    ((1, 64, 68, 2, 0, 1, 170, 40), (X3, 129, 2, 15, 16, 9, 1, 3)),    # empty split, circular
    # wgrad_x3_kernel<1, 1> (padded / circular, so not the wide kernel)
    ((1, 36, 68, 1, 1, 0, 9, 16), (X3, 3, 2, 1, 1, 3, 0, 3)),
    ((1, 68, 68, 1, 1, 0, 75, 40), (X3, 57, 4, 8, 8, 8, 1, 1)),
    ((1, 36, 68, 1, 0, 1, 50, 70), (X3, 65, 2, 9, 9, 8, 0, 1)),
    # wgrad1_wide_kernel
    ((1, 196, 388, 1, 0, 0, 3, 7), (WIDE1, 1, 6, 1, 1, 1, 0, 1)),      # one ragged tile (21 px), base 6
    ((1, 196, 196, 1, 0, 0, 5, 9), (WIDE1, 2, 4, 1, 1, 2, 0, 2)),
    ((1, 64, 64, 1, 0, 0, 9, 9), (WIDE1, 3, 1, 1, 1, 3, 0, 3)),
    ((1, 196, 196, 1, 0, 0, 45, 46), (WIDE1, 65, 4, 9, 9, 8, 0, 1)),
    ((1, 196, 196, 1, 0, 0, 57, 32), (WIDE1, 57, 4, 8, 8, 8, 1, 1)),
    ((1, 196, 388, 1, 0, 0, 64, 68), (WIDE1, 136, 6, 16, 16, 9, 1, 1)),  # 17 -> 16, base 6
    ((1, 196, 196, 1, 0, 0, 129, 32), (WIDE1, 129, 4, 15, 16, 9, 1, 3)),
    # wgrad2_wide_kernel
    ((1, 68, 68, 2, 0, 0, 2, 11), (WIDE2, 1, 1, 1, 1, 1, 0, 1)),
    ((1, 132, 132, 2, 1, 0, 6, 9), (WIDE2, 3, 4, 1, 1, 3, 0, 3)),
    ((1, 132, 132, 2, 1, 0, 25, 70), (WIDE2, 65, 4, 9, 9, 8, 0, 1)),
    ((1, 132, 132, 2, 0, 0, 38, 40), (WIDE2, 57, 4, 8, 8, 8, 1, 1)),
    ((2, 132, 196, 2, 0, 1, 34, 60), (WIDE2, 136, 4, 16, 16, 9, 1, 1)),
    ((1, 132, 132, 2, 0, 1, 86, 48), (WIDE2, 129, 4, 15, 16, 9, 1, 3)),
    # the 512-work-group grid (204 800 pixels) and the 256 one just under the threshold (199 680)
    ((2, 68, 68, 3, 1, 0, 320, 320), (X3, 3200, 4, 128, 128, 25, 1, 25)),
    ((2, 68, 68, 3, 1, 0, 312, 320), (X3, 3120, 4, 64, 64, 49, 1, 33)),
    ((2, 196, 196, 1, 0, 0, 320, 320), (WIDE1, 6400, 4, 128, 128, 50, 1, 50)),
    ((2, 132, 132, 2, 0, 0, 320, 320), (WIDE2, 6400, 4, 128, 128, 50, 1, 50)),
    ((2, 64, 132, 2, 0, 0, 320, 320), (X3, 3200, 3, 160, 168, 20, 1, 20)),  # 170 -> 168 rounding, 8 empty splits
]


def regime(pl):
    """A plan in REGIMES' form."""
    owning, last = last_owning(pl)
    return (pl.kernel, pl.ntiles, pl.base, owning, pl.splits, pl.per, pl.remap, last)


def args(B, M, N, k, pad, circ, Ha, Wa, a=0x1000, x=0x2000, g=0x3000):
    """nps_wgrad_t of a (B, M, N, k, pad, circ, Ha, Wa) case as ad.wgrad fills it (dummy pointers: host use only)."""
    import nps_hip
    p = nps_hip.WgradArgs()
    p.a, p.B, p.Ha, p.Wa, p.M = a, B, Ha, Wa, M
    p.x, p.Hx, p.Wx, p.N = x, Ha + k - 1 - 2 * pad - 2 * circ, Wa + k - 1 - 2 * pad - 2 * circ, N
    p.KH = p.KW = k
    p.dil, p.pad_y, p.pad_x, p.circ, p.g = 1, pad, pad, circ, g
    return p


def query(p):
    """The plan of a filled nps_wgrad_t, or None where the launch would refuse it."""
    import nps_hip
    out = (ctypes.c_int * 8)()
    if nps_hip.lib.nps_conv2d_wgrad_x3_plan(ctypes.byref(p), out) < 0:
        return None
    return Plan(*out)


def plan(B, M, N, k, pad, circ, Ha, Wa):
    return query(args(B, M, N, k, pad, circ, Ha, Wa))


def decode(pl, l):
    """(tile, split) of work-group l, as the kernels compute it from blockIdx.x."""
    if pl.remap:
        j = l >> 3  # this work-group's rank on its XCD (work-groups are dealt to the 8 XCDs round-robin)
        return j % pl.base, (j // pl.base) * 8 + (l & 7)
    return l % pl.base, l // pl.base


def owned(pl, split):
    """[t_begin, t_end) of a split; t_begin >= t_end is the kernels' early return."""
    t_begin = split * pl.per
    return t_begin, min(pl.ntiles, t_begin + pl.per)


def ref_wgrad(a, x, k, pad, circ):
    """G[m][n][ky][kx] = sum_{b,p} a[b][p][m] Xext[b][p + (ky, kx)][n] of NHWC a [B][Ha][Wa][M], x [B][Hx][Wx][N] in
    their own dtype (fp64: the reference), Xext = x extended circularly by circ, then by pad zeros: k * k matmuls
    over shifted slices — what torch.nn.grad.conv2d_weight computes, at a cost a 200 000-pixel case can afford."""
    import torch
    import torch.nn.functional as F
    B, Ha, Wa, M = a.shape
    N = x.shape[3]
    if circ:
        x = torch.cat([x[:, -circ:], x, x[:, :circ]], 1)
        x = torch.cat([x[:, :, -circ:], x, x[:, :, :circ]], 2)
    if pad:
        x = F.pad(x, (0, 0, pad, pad, pad, pad))
    assert x.shape[1:3] == (Ha + k - 1, Wa + k - 1)
    at = a.reshape(-1, M).T.contiguous()
    g = torch.empty(M, N, k, k, dtype=a.dtype)
    for ky in range(k):
        for kx in range(k):
            g[:, :, ky, kx] = at @ x[:, ky:ky + Ha, kx:kx + Wa].reshape(-1, N)
    return g


def last_owning(pl):
    """(number of splits that own a tile, tile count of the last of them)"""
    n = -(-pl.ntiles // pl.per)
    t0, t1 = owned(pl, n - 1)
    return n, t1 - t0
