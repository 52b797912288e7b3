"""Shared pieces of the per-cloud + per-point layer tests (tests/test_cloudpoint_ref_cpu.py, tests/test_cloudpoint_paths_gpu.py,
tests/test_pointnet_seg_gpu.py): the case tables, the inputs, the split rule of the backward restated, and the family's
relative-RMS bar.  The guarded output buffer, the per-element bound and its constants are those of tests/edge_checks.py,
imported and unchanged.  Nothing here touches the library.  Inputs are drawn on the CPU from a generator seeded by the case
and then moved, so every file sees the same numbers."""
import zlib

import torch

import edge_checks as K
from edge_checks import C_BOUND, U, Out, bits_equal  # noqa: F401  (re-exported to the test files)

# Relative RMS against float64 of an fp32 evaluation of every definition, SEQUENTIAL (one fp32 accumulator per element, terms
# in index order, a multiplication and an addition rounded separately), on the inputs below
# (tests/test_cloudpoint_ref_cpu.py::test_fp32_sequential prints these and holds the constant to them; largest per output over
# its cases):
#   fwd Y      1.14e-07 at (1, 16, 128)
#   fwd S1     6.28e-07 at (1, 1, 64)
#   fwd S2     7.45e-07 at (1, 1, 64)
#   bwd dX     4.81e-07 at (3, 1, 1024)
#   bwd dWx    2.70e-06 at (260, 130, 64)
#   bwd dCtr   4.53e-07 at (1, 1030, 64)
# dWx over 33 800 rows sets the bar: a sequential chain's error grows with the root of its length.  (The statistics of a single
# row are the next largest: y - pivot is a small difference of two numbers of the size of the mean.)  The family's bar is twice
# the largest value; the factor leaves room for the tiled order of the MFMA accumulation and of the split sums where it
# differs from the sequential one.
RMS_FP32_SEQUENTIAL_WORST = 2.70e-6
RMS_BAR = 2 * RMS_FP32_SEQUENTIAL_WORST

K_WIDTH = 64
POINT_TILE = 64          # points per step of the backward; a split is a whole number of them
FWD_POINTS = 128         # points per workgroup of the forward = rows of one statistics partial
SPLIT_CAP = 16
TARGET_WGS = 512
CHANNEL_CHUNK = 64       # channels per chunk; the backward's passes take 8, 4, 2 or 1 chunks, greedily


def check_sum(out, triple, what, report=None):
    """edge_checks.check_sum itself -- |out - ref| <= C (L + 4) 2^-24 A per element -- with this family's RMS bar"""
    prev, K.RMS_BAR = K.RMS_BAR, RMS_BAR
    try:
        K.check_sum(out, triple, what, report=report)
    finally:
        K.RMS_BAR = prev


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def bwd_splits(b, n):
    """pcops.h: the largest power of two <= min(ceil(512 / b), ceil(n / 64), 16)"""
    want = min(-(-TARGET_WGS // b), -(-n // POINT_TILE), SPLIT_CAP)
    s = 1
    while 2 * s <= want:
        s *= 2
    return s


def bwd_chunk(n, splits):
    """points per split: ceil(n / splits) rounded up to whole 64-point steps"""
    return -(-(-(-n // splits)) // POINT_TILE) * POINT_TILE


def ws_floats(b, n, c):
    """pcops.h: [parts][64][c] where there is more than one part, then [parts][c] where a cloud has more than one split"""
    s = bwd_splits(b, n)
    parts = b * s
    return (parts * K_WIDTH * c if parts > 1 else 0) + (parts * c if s > 1 else 0)


def passes(c):
    """the backward's channel passes, in chunks: 8, 4, 2 or 1, greedily"""
    left, out = c // CHANNEL_CHUNK, []
    while left:
        out.append(8 if left >= 8 else 4 if left >= 4 else 2 if left >= 2 else 1)
        left -= out[-1]
    return out


# (b, n, c).  n: 1, one on either side of the 16-point MFMA tile, of the backward's 64-point step and of the forward's
# 128-point workgroup, 257.  b: 1, 2, 3 -- a neighbouring cloud's Ctr row or dCtr sum shows.  c: 64 (one chunk), 128, 512 (one
# full pass), 1024 (two passes, dX of the second added to the first's); the chunks are 64 wide, so 576 is no special width
# for them, but the PASSES make it one (8 + 1 chunks), and 960 runs every pass size (8 + 4 + 2 + 1).
CASES = [
    (1, 1, 64),          # the smallest shape: one point, one wave at work, direct store of dWx and dCtr
    (1, 15, 64),
    (1, 16, 128),
    (1, 17, 64),         # a second wave's tile with one point
    (1, 63, 128),
    (1, 64, 64),
    (1, 65, 512),        # 2 splits of 64, the second holds one point: two parts
    (1, 127, 64),
    (1, 128, 128),
    (1, 129, 1024),      # a second forward workgroup with one point; two passes
    (2, 129, 576),       # passes of 8 and 1 chunks
    (3, 17, 960),        # passes of 8, 4, 2 and 1 chunks; three clouds, one split each: three parts
    (3, 70, 128),        # clouds that differ; 2 splits of 64 per cloud
    (2, 64, 512),
    (1, 257, 512),       # 5 steps: 4 splits of 128 points, the last holds no point
    (2, 257, 64),
    (3, 1, 1024),        # one point per cloud
]
# ((b, n, c), parts = b splits, splits per cloud that hold points).  One part, two, the cap of 16 splits, and splits that hold
# no row (the rule CAN produce them: the chunk is rounded up to whole 64-point steps).
PARTS_CASES = [
    ((1, 1, 64), 1, 1),
    ((1, 64, 64), 1, 1),
    ((1, 65, 512), 2, 2),
    ((3, 17, 960), 3, 1),
    ((3, 70, 128), 6, 2),
    ((1, 257, 512), 4, 3),       # 4 splits of 128 points, the last holds no point and stores zeros
    ((2, 257, 64), 8, 3),
    ((1, 520, 64), 8, 5),        # 9 steps: 8 splits of 128, three of them empty
    ((2, 1024, 64), 32, 16),     # the cap: 16 splits of exactly 64 points
    ((1, 1030, 64), 16, 9),      # 17 steps: the cap, splits of 128, seven of them empty
    ((260, 130, 64), 520, 2),    # the cloud count caps it: ceil(512 / 260) = 2 although there are 3 steps
]
UNSUPPORTED = [(1, 20, 32, 128), (1, 20, 64, 96), (1, 20, 64, 1088), (1, 20, 64, 0), (1, 0, 64, 64)]       # (b, n, k, c)


def all_cases():
    return CASES + [c for c, _, _ in PARTS_CASES if c not in CASES]


def case_id(case):
    case = case[0] if isinstance(case[0], tuple) else case
    return "_".join(str(v) for v in case)


def inputs(case, device="cpu"):
    """X, Wx, Ctr, pivot, G, Y, p, q, t for (b, n, c).  The tensors that are summed carry a per-column offset of 0.25 .. 0.75
    so that no sum cancels to zero; the pivot lies within a standard deviation or so of the column means of X Wx + Ctr (as a
    moving mean does); Y of the backward is an input like any other."""
    b, n, c = case
    g_ = gen("cloudpoint", case)

    def off(w):
        return 0.25 + 0.5 * torch.rand(w, generator=g_)

    X = torch.randn(b * n, K_WIDTH, generator=g_) + off(K_WIDTH)
    Wx = (torch.randn(K_WIDTH, c, generator=g_) + off(c)) / 8.0
    Ctr = torch.randn(b, c, generator=g_) + off(c)
    pivot = (X.double().mean(0) @ Wx.double() + Ctr.double().mean(0)).float() + 0.5 * torch.randn(c, generator=g_)
    G = torch.randn(b * n, c, generator=g_) + off(c)
    Y = torch.randn(b * n, c, generator=g_) + off(c)
    p = 0.5 + torch.rand(c, generator=g_)
    q = 0.2 * torch.rand(c, generator=g_) + 0.05
    t = 0.2 * torch.rand(c, generator=g_) + 0.05
    return tuple(v.to(device).contiguous() for v in (X, Wx, Ctr, pivot, G, Y, p, q, t))
