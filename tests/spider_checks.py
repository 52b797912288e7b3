"""Shared pieces of the SpiderConv reference tests (tests/test_spider_ref_cpu.py, tests/test_spider_paths_gpu.py): the case
tables, the inputs both files build, and the family's relative-RMS bar.  The guarded output buffer, the per-element bound
and its constants are those of tests/edge_checks.py, imported and unchanged.  Nothing here touches the library.  Inputs are
always drawn on the CPU from a generator seeded by the case and then moved, so both files see the same numbers."""
import zlib

import numpy as np
import torch

import edge_checks as K
from edge_checks import C_BOUND, U, Out, bits_equal  # noqa: F401  (re-exported to the two test files)

T = 5
EPS = float(np.float32(1e-6))      # the eps the kernel is handed (a C float), widened

# Relative RMS against float64 of an fp32 evaluation of every definition, SEQUENTIAL in the header's order, on the inputs
# below (tests/test_spider_ref_cpu.py::test_fp32_* print these; largest per entry point over its cases):
#   taylor_fwd g 1.29e-07 (rows = 1)
#   taylor_bwd dtheta 1.02e-05 (rows = 3 * 65536 + 5), dtbias 5.31e-06 (rows = 65536 + 77)
#   conv_fwd y 2.36e-06 (1, 130, 20, 256, 256: 25 601 terms)
#   conv_wgrad dw 4.83e-07, db 4.97e-07 (2, 520, 4, 3, 16: 1040 rows)
#   conv_dgrad dfg 2.10e-07, dg 2.36e-07 (1, 96, 3, 256, 512)     scatter_grouped dF 4.86e-08 (3, 65, 7, 17, 48)
#   group norm mean 8.07e-07, var 1.39e-06 (2, 40, 512, 2: 10 240 terms), out 5.35e-08 (2, 300, 80, 16)
#   group norm backward dgamma 3.07e-07, dbeta 3.28e-07 (2, 300, 80, 16), m1 7.85e-07, m2 1.22e-06 (2, 40, 512, 2),
#   dx 5.93e-08 (2, 70, 16, 16)
# edge_checks.RMS_BAR = 1e-6 was set for sums of a few hundred terms; the sums here have up to 196 613.  The family's bar is
# twice the largest value above; the factor of two leaves room for the chunked order of the MFMA accumulation and of the
# block reductions where it differs from the sequential one.
RMS_FP32_SEQUENTIAL_WORST = 1.02e-5
RMS_BAR = 2 * RMS_FP32_SEQUENTIAL_WORST


def check_sum(out, triple, what, report=None, rms=True):
    """edge_checks.check_sum itself -- |out - ref| <= C (L + 4) 2^-24 A per element -- with this family's RMS bar.
    rms=False: the per-element bound alone, for a sum that is zero in exact arithmetic (the column sums of a group-norm
    gradient with one channel per group), where a ratio to the norm of the reference says nothing"""
    prev, K.RMS_BAR = K.RMS_BAR, RMS_BAR if rms else float("inf")
    try:
        K.check_sum(out, triple, what, report=report)
    finally:
        K.RMS_BAR = prev


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------------------- contraction
# (b, n, k, C, O), splits of the weight gradient, splits that hold rows -- from wgrad_splits() of csrc/spider.hip
CONV_CASES = [
    ((1, 40, 5, 3, 16), 1, 1),         # one partial row tile; C < 16; O = 16; b n <= 64: one split, dw / db stored directly
    ((2, 64, 1, 16, 64), 2, 2),        # whole tiles only; k = 1; C = 16 exactly
    ((3, 65, 7, 17, 48), 4, 4),        # one-row tail tile; channel tail of 1; O = 48; wgrad tiles straddle clouds; 3-row split
    ((2, 300, 20, 40, 80), 9, 5),      # ragged; four trailing splits without rows store zeros
    ((1, 130, 20, 256, 256), 1, 1),    # C = 256; one split because the grid already has 1280 workgroups; 3 row tiles
    ((2, 520, 4, 3, 16), 16, 9),       # the cap of 16 splits, 7 of them empty
    ((1, 70, 64, 5, 32), 2, 2),        # k = 64
    ((1, 96, 3, 256, 512), 2, 2),      # O = 512: eight column tiles
]
END_TO_END = [(3, 65, 7, 17, 48), (1, 40, 5, 3, 16)]


def conv_id(case):
    return "b%d_n%d_k%d_c%d_o%d" % tuple(case[0] if isinstance(case[0], tuple) else case)


def wgrad_chunk(b, n, splits):
    """rows per split: the launcher rounds ceil(b n / splits) up to whole 64-row tiles"""
    per = -(-(b * n) // splits)
    return -(-per // 64) * 64


def conv_inputs(shape, device="cpu"):
    """feat (b, n, C), idx (b, n, k) random in [0, n) per cloud (repeats, clouds that differ, NOT self-first), g, w, bias,
    dy; feat, g, w and dy carry a per-column offset of 0.25 .. 0.75 so that no sum cancels to zero"""
    b, n, k, c, o = shape
    g_ = gen("conv", shape)

    def off(m):
        return 0.25 + 0.5 * torch.rand(m, generator=g_)

    feat = torch.randn(b, n, c, generator=g_) + off(c)
    idx = torch.randint(0, n, (b, n, k), generator=g_, dtype=torch.int32)
    g = 0.5 * torch.randn(b, n, k, T, generator=g_) + off(T)
    w = (torch.randn(k * c * T, o, generator=g_) + off(o)) / float(np.sqrt(k * c))
    bias = 0.1 * torch.randn(o, generator=g_) + 0.05
    dy = torch.randn(b, n, o, generator=g_) + off(o)
    return tuple(t.to(device).contiguous() for t in (feat, idx, g, w, bias, dy))


# --------------------------------------------------------------------------------------------------------------- Taylor
# one thread; one block less a thread, exactly, plus a thread; the 256 x 256 grid exactly full; a ragged second trip that
# 77 threads take; several trips
TAYLOR_ROWS = [1, 255, 256, 257, 65536, 65536 + 77, 3 * 65536 + 5]


def taylor_inputs(rows, device="cpu"):
    """delta (rows, 3) in [-0.3, 0.3]^3 with every seventh row exactly zero, theta, tbias, dg with a non-zero mean"""
    g_ = gen("taylor", rows)
    delta = 0.6 * torch.rand(rows, 3, generator=g_) - 0.3
    delta[3::7] = 0.0
    theta = 0.5 * torch.randn(19, T, generator=g_)
    tbias = 0.2 * torch.randn(T, generator=g_)
    dg = torch.randn(rows, T, generator=g_) + (0.25 + 0.5 * torch.rand(T, generator=g_))
    return tuple(t.to(device).contiguous() for t in (delta, theta, tbias, dg))


# ------------------------------------------------------------------------------------------------------ group norm + ReLU
# (b, n, C, groups)
GN_CASES = [
    (2, 70, 16, 16),       # cg = 1
    (3, 33, 48, 16),       # cg = 3: nact = 255
    (2, 50, 112, 16),      # cg = 7: nact = 252
    (2, 300, 80, 16),      # cg = 5
    (1, 9, 16, 1),         # one group, n cg = 144 < 256: idle threads in both reductions
    (2, 40, 512, 2),       # cg = 256, the limit
    (2, 130, 256, 16),     # the model's last layer
    (2, 32, 32, 4),        # cg = 8, n cg = 256 = 2^8: the case with the constant group
]
GN_CONST = {(2, 32, 32, 4): (1, 1, 1.5)}      # shape -> (cloud, group, v): every x of that (cloud, group) is v


def gn_inputs(shape, device="cpu"):
    """x with a per-channel scale and offset, gamma of either sign, beta, dout.  The last channel has gamma = 0 and
    beta = 0: its output is exactly 0 and, by the kernel's y > 0 rule, so is its gy.  The shape in GN_CONST has one
    (cloud, group) whose x all equal v = 1.5 with n cg a power of two: every partial sum of its fp32 mean is a small
    multiple of 1.5 and exact, so mean = v to the last bit, every deviation is 0, var = 0, rstd = 1 / sqrt(eps), and
    out = relu(beta) exactly."""
    b, n, c, groups = shape
    g_ = gen("gn", shape)
    x = torch.randn(b, n, c, generator=g_) * (0.5 + torch.rand(c, generator=g_)) + torch.randn(c, generator=g_)
    gamma = 0.5 + torch.rand(c, generator=g_)
    gamma[torch.arange(c) % 3 == 1] *= -1.0
    beta = 0.2 * torch.randn(c, generator=g_)
    gamma[c - 1], beta[c - 1] = 0.0, 0.0
    dout = torch.randn(b, n, c, generator=g_)
    if shape in GN_CONST:
        cloud, grp, v = GN_CONST[shape]
        cg = c // groups
        x[cloud, :, grp * cg:(grp + 1) * cg] = v
    return tuple(t.to(device).contiguous() for t in (x, gamma, beta, dout))
