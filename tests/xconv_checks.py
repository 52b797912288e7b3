"""Shared pieces of the X-Conv reference tests (tests/test_xconv_ref_cpu.py, tests/test_xconv_paths_gpu.py,
tests/test_pointcnn_gpu.py): the case tables, the inputs, and the family's relative-RMS bar.  The guarded output buffer, the
per-element bound and its constants are those of tests/edge_checks.py, imported and unchanged.  Nothing here touches the
library.  Inputs are drawn on the CPU from a generator seeded by the case and then moved, so every file sees the same numbers."""
import zlib

import torch

import edge_checks as K
from edge_checks import C_BOUND, U, Out, bits_equal  # noqa: F401  (re-exported to the test files)

# Relative RMS against float64 of an fp32 evaluation of every definition, SEQUENTIAL (one fp32 accumulator per element, terms
# in index order), on the inputs below (tests/test_xconv_ref_cpu.py::test_fp32_sequential prints these; largest per entry
# point over its cases):
#   fwd out 8.11e-08 (2, 40, 17, 12, 12, 48, 2)
#   dgrad dX 2.38e-07, dlifted 7.39e-08, dfts_grouped 7.38e-08 (3, 20, 20, 16, 48, 192, 2: 240 channels)
#   wgrad dwd 4.92e-07 (8, 130, 130, 2, 100, 30, 1: 1040 points)
#   scatter dfts 6.69e-08 (3, 20, 20, 16, 48, 192, 2)
# The family's bar is twice the largest value; the factor leaves room for the tiled order of the MFMA accumulation and of the
# split sums where it differs from the sequential one.
RMS_FP32_SEQUENTIAL_WORST = 4.92e-7
RMS_BAR = 2 * RMS_FP32_SEQUENTIAL_WORST


def check_sum(out, triple, what, report=None):
    """edge_checks.check_sum itself -- |out - ref| <= C (L + 4) 2^-24 A per element -- with this family's RMS bar"""
    prev, K.RMS_BAR = K.RMS_BAR, RMS_BAR
    try:
        K.check_sum(out, triple, what, report=report)
    finally:
        K.RMS_BAR = prev


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# (b, n, p, K, c1, c2, dm)
CASES = [
    (1, 33, 33, 8, 24, 0, 4),        # no fts; dm = 4; a one-row tail of a 16-point workgroup and of a 32-point split
    (2, 40, 17, 12, 12, 48, 2),      # K < 16: the padding contributes zero; the lifted / fts split inside a tile; c = 60; p != n
    (3, 20, 20, 16, 48, 192, 2),     # K = 16 exactly; c = 240; clouds that differ
    (1, 9, 5, 1, 3, 5, 1),           # K = 1; dm = 1; channel tails only
    (2, 64, 64, 5, 16, 16, 3),       # odd K; whole tiles; an odd multiplier
]
# (shape, splits of the weight gradient, splits that hold points) -- wgrad_splits() / wgrad_chunk() of csrc/xconv.hip: the
# largest power of two <= min(ceil(512 / channel tiles), b p / 16, 64), each split a whole number of 16-point steps
WGRAD_CASES = [
    ((1, 1, 1, 1, 1, 0, 1), 1, 1),           # the smallest shape: one point, one channel, direct store, no workspace
    ((1, 9, 5, 1, 3, 5, 1), 1, 1),           # fewer than 32 points: one split
    ((1, 33, 33, 8, 24, 0, 4), 2, 2),        # 2 splits of 32 points: the second holds one
    ((2, 40, 17, 12, 12, 48, 2), 2, 2),
    ((3, 20, 20, 16, 48, 192, 2), 2, 2),     # the splits straddle the cloud boundaries at points 20 and 40
    ((2, 35, 35, 3, 4, 3, 1), 4, 3),         # 70 points, 4 splits of 32: the last one holds no point and stores zeros
    ((2, 64, 64, 5, 16, 16, 3), 8, 8),       # 8 splits of exactly 16 points
    ((2, 130, 130, 4, 8, 8, 2), 16, 9),      # 16 splits of 32 points, 7 of them empty
    ((1, 520, 520, 2, 3, 2, 1), 32, 17),     # 32 splits, 15 of them empty
    ((8, 130, 130, 2, 100, 30, 1), 32, 22),  # 1040 points but 9 channel tiles: ceil(512 / 9) = 57 caps the count at 32;
                                             # splits of 48 points, 10 of them empty
    ((1, 1030, 1030, 2, 2, 1, 1), 64, 33),   # the cap of 64 splits, 31 of them empty
]
UNSUPPORTED = [
    (1, 20, 20, 17, 8, 8, 1),        # K > 16
    (1, 20, 20, 4, 8, 8, 5),         # dm > 4
    (1, 20, 20, 4, 200, 124, 3),     # c dm = 972 > 960
]


def case_id(case):
    return "b%d_n%d_p%d_k%d_c%d+%d_dm%d" % tuple(case[0] if isinstance(case[0], tuple) else case)


def wgrad_chunk(b, p, splits):
    per = -(-(b * p) // splits)
    return -(-per // 16) * 16


def inputs(shape, device="cpu"):
    """lifted, fts (None with c2 == 0), idx random in [0, n) per cloud with repeats, X, wd, dout; every float tensor carries a
    per-column offset of 0.25 .. 0.75 so that no sum cancels to zero"""
    b, n, p, k, c1, c2, dm = shape
    g_ = gen("xconv", shape)
    c = c1 + c2

    def off(m):
        return 0.25 + 0.5 * torch.rand(m, generator=g_)

    lifted = torch.randn(b, p, k, c1, generator=g_) + off(c1)
    fts = torch.randn(b, n, c2, generator=g_) + off(c2) if c2 else None
    idx = torch.randint(0, n, (b, p, k), generator=g_, dtype=torch.int32)
    X = (torch.randn(b, p, k, k, generator=g_) + off(k)) / float(k) ** 0.5
    wd = (torch.randn(k, c, dm, generator=g_) + off(dm)) / float(k) ** 0.5
    dout = torch.randn(b, p, c * dm, generator=g_) + off(c * dm)
    return tuple(t.to(device).contiguous() if t is not None else None for t in (lifted, fts, idx, X, wd, dout))


def small_setting():
    """four X-Conv layers on 64 points with K D no larger than the previous layer's point count; the shapes of
    modelnet_x3_l4 scaled down: a first layer without fts and dm = 4, sampling, a repeated P, dilation 1, 2 and 3"""
    from scanobjectnn_amd.pointcnn import settings as S
    return S.make(xconv_params=S.xconv_params([(4, 1, -1, 16, []), (6, 2, 24, 32, []), (8, 2, 16, 64, []),
                                               (5, 3, 16, 128, [])]),
                  fc_params=S.fc_params([(64, 0.0), (32, 0.8)]), with_global=True, sampling='random',
                  with_X_transformation=True, sorting_method=None)


def randomise(net, seed):
    """gammas, betas and moving statistics off their initial 1 / 0 so that no term of the definition is trivially right"""
    g_ = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, v in net.state_dict().items():
            r = torch.rand(v.shape, generator=g_).to(v.device, v.dtype)
            if name.endswith("/gamma") or name.endswith("/moving_variance"):
                v.copy_(0.5 + r)
            elif name.endswith("/beta") or name.endswith("/moving_mean") or name.endswith("/bias"):
                v.copy_(0.4 * r - 0.2)
