"""Shared pieces of the per-cloud transform tests (tests/test_tnet_ref_cpu.py, tests/test_tnet_paths_gpu.py,
tests/test_pointnet_gpu.py): the case tables, the inputs, the split rule of the backward restated, and the family's
relative-RMS bar.  The guarded output buffer, the per-element bound and its constants are those of tests/edge_checks.py,
imported and unchanged.  Nothing here touches the library.  Inputs are drawn on the CPU from a generator seeded by the case
and then moved, so every file sees the same numbers."""
import zlib

import torch

import edge_checks as K
from edge_checks import C_BOUND, U, Out, bits_equal  # noqa: F401  (re-exported to the test files)

# Relative RMS against float64 of an fp32 evaluation of every definition, SEQUENTIAL (one fp32 accumulator per element, terms
# in index order), on the inputs below (tests/test_tnet_ref_cpu.py::test_fp32_sequential prints these; largest per output
# over its cases):
#   fwd out          1.42e-07 at (1, 1)
#   bwd dX           1.34e-07 at (1, 17)
#   bwd dT           4.72e-07 at (2, 1024)
#   ortho dT         1.27e-06 at (3, 'near')
#   ortho loss_parts 9.16e-07 at (32, 'near')
# The regulariser sets the bar: T T^T - I is the small difference (about 1e-2) of sums that reach 1, so the 64 roundings of
# the sum are about 1e-6 of what is left.  The family's bar is twice the largest value; the factor leaves room for the tiled
# order of the MFMA accumulation and of the split sums where it differs from the sequential one.
RMS_FP32_SEQUENTIAL_WORST = 1.27e-6
RMS_BAR = 2 * RMS_FP32_SEQUENTIAL_WORST

K_WIDTH = 64
POINT_TILE = 64          # points per step of the backward; a split is a whole number of them (the forward's MFMA tile is 16
FWD_POINTS = 128         # points, its workgroup 128)
SPLIT_CAP = 16
TARGET_WGS = 512


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


# (b, n): the transform forward and backward
CASES = [
    (1, 1),          # the smallest shape: one point, one wave at work, direct store of dT
    (1, 15),         # one below the 16-point MFMA tile
    (1, 16),
    (1, 17),         # a second wave with one point
    (1, 63),         # one below the backward's step
    (1, 64),
    (1, 65),         # one above the size of a split: 2 splits of 64, the second holds one point
    (1, 127),        # one below the forward's workgroup
    (1, 128),
    (1, 129),        # a second forward workgroup with one point; 2 splits of 128, the second holds one point
    (3, 70),         # clouds and transforms that differ; 2 splits of 64 per cloud
]
# ((b, n), splits of the backward, splits that hold points)
SPLIT_CASES = [
    ((1, 1), 1, 1),
    ((1, 64), 1, 1),
    ((1, 65), 2, 2),
    ((1, 129), 2, 2),
    ((3, 70), 2, 2),
    ((1, 257), 4, 3),        # 5 steps: 4 splits of 128 points, the last holds no point and stores zeros
    ((1, 520), 8, 5),        # 9 steps: 8 splits of 128, three of them empty
    ((2, 1024), 16, 16),     # the cap: 16 splits of exactly 64 points
    ((1, 1030), 16, 9),      # 17 steps: the cap, splits of 128, seven of them empty
    ((260, 130), 2, 2),      # the cloud count caps it: ceil(512 / 260) = 2 although there are 3 steps
]
UNSUPPORTED = [(1, 20, 32), (1, 20, 65), (1, 0, 64)]       # (b, n, k)
# (b, kind): the regulariser; 'near' = an orthogonal matrix plus a perturbation of about 1e-2, as in training
ORTHO_CASES = [(1, "near"), (3, "near"), (32, "near"), (2, "random")]


def case_id(case):
    case = case[0] if isinstance(case[0], tuple) else case
    return "_".join(str(v) for v in case)


def inputs(shape, device="cpu"):
    """X, T, G for (b, n); every tensor carries a per-column offset of 0.25 .. 0.75 so that no sum cancels to zero"""
    b, n = shape
    g_ = gen("tnet", shape)

    def off():
        return 0.25 + 0.5 * torch.rand(K_WIDTH, generator=g_)

    X = torch.randn(b, n, K_WIDTH, generator=g_) + off()
    T = (torch.randn(b, K_WIDTH, K_WIDTH, generator=g_) + off()) / 8.0
    G = torch.randn(b, n, K_WIDTH, generator=g_) + off()
    return tuple(t.to(device).contiguous() for t in (X, T, G))


def ortho_inputs(case, device="cpu"):
    b, kind = case
    g_ = gen("ortho", case)
    if kind == "random":
        T = (torch.randn(b, K_WIDTH, K_WIDTH, generator=g_) + 0.25 + 0.5 * torch.rand(K_WIDTH, generator=g_)) / 8.0
    else:
        q, _ = torch.linalg.qr(torch.randn(b, K_WIDTH, K_WIDTH, generator=g_, dtype=torch.float64))
        T = (q + 1e-2 * torch.randn(b, K_WIDTH, K_WIDTH, generator=g_, dtype=torch.float64)).float()
    return T.to(device).contiguous()


def randomise(net, seed):
    """gammas, betas, biases and moving statistics off their initial 1 / 0 so that no term of the definition is trivially
    right; the T-Net heads' zero weights become small, so that the transforms differ from cloud to cloud"""
    g_ = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, v in net.state_dict().items():
            r = torch.rand(v.shape, generator=g_).to(v.device, v.dtype)
            if name.endswith("/gamma") or name.endswith("/moving_variance"):
                v.copy_(0.5 + r)
            elif name.endswith("/beta") or name.endswith("/moving_mean") or name.endswith("/biases"):
                v.add_(0.4 * r - 0.2)
            elif "transform_" in name and name.endswith("/weights") and v.dim() == 2 and v.abs().max() == 0:
                v.copy_(0.02 * r - 0.01)
