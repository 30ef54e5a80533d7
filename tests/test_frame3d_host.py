"""CPU checks of the 3-D frame kernels' index arithmetic and host refusals (csrc/frame3d_bwd.hip).

nps_frame3d_locate runs the same __host__ __device__ voxel decode as nps_frame3d_fwd / nps_frame3d_bwd /
nps_add_at_copy3d, so an index slip shows here and not as a fault on the GPU.  The reference is the index arithmetic
of torch's slicing: models.common.crop_Nd's construction (a zero frame, the overlapping slices assigned) on three
axes, applied to a volume that holds its own linear voxel numbers."""
import ctypes
import itertools

import pytest
import torch

FRAME = (5, 6, 7)


def _args(srcs, frame=FRAME, B=2, groups=0, bf16=0, pre_act=0):
    """Conv3dArgs of a frame with dummy (never dereferenced) pointers.  srcs: [(C, (D, H, W), (od, oh, ow))]."""
    import nps_hip
    a = nps_hip.Conv3dArgs()
    a.nsrc = len(srcs)
    for i, (C, dhw, off) in enumerate(srcs):
        a.src[i].ptr = 0x1000 * (i + 1)
        a.src[i].C, (a.src[i].D, a.src[i].H, a.src[i].W) = C, dhw
        a.src[i].off_d, a.src[i].off_h, a.src[i].off_w = off
    a.B, (a.Dc, a.Hc, a.Wc), a.Cin = B, frame, sum(s[0] for s in srcs)
    if groups:
        a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_groups, a.gn_eps = 0x8000, 0x9000, 0xa000, groups, 1e-5
    a.pre_act, a.bf16 = pre_act, bf16
    return a


def _crop_ref(n, off, f):
    """Per axis, as crop_Nd slices: frame range [f0, f1) <- source range [f0 - off, f1 - off)."""
    f0, f1 = max(0, off), min(f, off + n)
    return f0, f1


def _reference_map(dhw, off, frame=FRAME):
    """frame-sized int tensor: the linear source voxel number that lands on each frame voxel, -1 where none does."""
    D, H, W = dhw
    src = torch.arange(D * H * W).view(D, H, W)
    out = torch.full(frame, -1, dtype=torch.long)
    (d0, d1), (h0, h1), (w0, w1) = (_crop_ref(n, o, f) for n, o, f in zip(dhw, off, frame))
    if d1 > d0 and h1 > h0 and w1 > w0:
        out[d0:d1, h0:h1, w0:w1] = src[d0 - off[0]:d1 - off[0], h0 - off[1]:h1 - off[1], w0 - off[2]:w1 - off[2]]
    return out


def _sweep(lib, a, si, dhw):
    """{source voxel number: frame voxel number} of the voxels nps_frame3d_locate places inside the frame."""
    fd, fh, fw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    got = {}
    D, H, W = dhw
    for d in range(D):
        for h in range(H):
            for w in range(W):
                rc = lib.nps_frame3d_locate(ctypes.byref(a), si, d, h, w, ctypes.byref(fd), ctypes.byref(fh),
                                            ctypes.byref(fw))
                assert rc in (0, 1), lib.nps_last_error().decode()
                if rc == 1:
                    assert 0 <= fd.value < a.Dc and 0 <= fh.value < a.Hc and 0 <= fw.value < a.Wc
                    got[(d * H + h) * W + w] = (fd.value * a.Hc + fh.value) * a.Wc + fw.value
    return got


# per axis every (size, offset) pair of {3, 5, 8} x {-2 .. 2}; the three axes take different pairs (rotations of
# the same list), so each pair meets each axis and the sizes and offsets are distinct per axis within a case
AXIS = list(itertools.product((3, 5, 8), (-2, -1, 0, 1, 2)))


@pytest.mark.parametrize("k", range(len(AXIS)))
def test_locate_matches_torch_slicing(k):
    import nps_hip
    lib = nps_hip.lib
    pairs = [AXIS[k], AXIS[(k + 4) % len(AXIS)], AXIS[(k + 8) % len(AXIS)]]
    dhw, off = tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)
    # the swept source sits last of three, behind two of other shapes: per-source tables must be indexed
    srcs = [(16, FRAME, (0, 0, 0)), (8, (7, 9, 8), (-1, -2, 0)), (4, dhw, off)]
    a = _args(srcs)
    ref = _reference_map(dhw, off)
    want = {int(s): i for i, s in enumerate(ref.reshape(-1).tolist()) if s >= 0}
    assert _sweep(lib, a, 2, dhw) == want
    ref1 = _reference_map((7, 9, 8), (-1, -2, 0))
    assert _sweep(lib, a, 1, (7, 9, 8)) == {int(s): i for i, s in enumerate(ref1.reshape(-1).tolist()) if s >= 0}
    assert len(_sweep(lib, a, 0, FRAME)) == 5 * 6 * 7


def test_locate_refuses_bad_queries():
    import nps_hip
    lib = nps_hip.lib
    a = _args([(16, FRAME, (0, 0, 0))])
    out = [ctypes.byref(ctypes.c_int()) for _ in range(3)]
    assert lib.nps_frame3d_locate(ctypes.byref(a), 1, 0, 0, 0, *out) < 0       # no such source
    assert lib.nps_frame3d_locate(ctypes.byref(a), 0, 5, 0, 0, *out) < 0       # voxel outside the source
    assert lib.nps_frame3d_locate(ctypes.byref(a), 0, 4, 5, 6, *out) == 1


ONE = [(16, FRAME, (0, 0, 0))]


@pytest.mark.parametrize("kw,null_gy,word", [
    (dict(srcs=ONE, bf16=1), False, "fp32 only"),
    (dict(srcs=ONE), True, "null"),
    (dict(srcs=[(18, FRAME, (0, 0, 0))], groups=4), False, "GroupNorm"),   # 18 % 4 != 0
    (dict(srcs=[]), False, "nsrc 0"),
], ids=["bf16", "null_gy", "groups", "nsrc0"])
def test_frame3d_bwd_host_refusals(kw, null_gy, word):
    """Refused before any HIP call (dummy pointers, NULL stream, no GPU): rc < 0 and a message naming the cause."""
    import nps_hip
    lib = nps_hip.lib
    a = _args(**kw)
    dsrc = (ctypes.c_void_p * 3)(0x4000, None, None)
    rc = lib.nps_frame3d_bwd(ctypes.byref(a), None if null_gy else 0x2000, None, dsrc, 0x5000, 0x6000, 0x7000, None)
    assert rc < 0
    assert word in lib.nps_last_error().decode()
    if not null_gy:
        assert lib.nps_frame3d_fwd(ctypes.byref(a), 0x2000, None) < 0
        assert word in lib.nps_last_error().decode()


def test_add_at_copy3d_host_refusals():
    import nps_hip
    lib = nps_hip.lib
    assert lib.nps_add_at_copy3d(None, 0x1000, 0x2000, 2, 5, 6, 7, 3, 4, 9, 16, 1, 1, -1, None) < 0
    assert lib.nps_add_at_copy3d(0x3000, 0x1000, 0x2000, 2, 5, 6, 7, 3, 4, 9, 0, 1, 1, -1, None) < 0
