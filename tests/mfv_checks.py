"""Shared pieces of the 3DmFV-Net reference tests (tests/test_mfv_ref_cpu.py, tests/test_mfv_paths_gpu.py,
tests/test_mfv3d_gpu.py): the case tables, the inputs all files build, and the family's bars.  The guarded output buffer, the
per-element bound and its constants are those of tests/edge_checks.py, imported and unchanged.  Nothing here touches the
library.  Inputs are always drawn on the CPU from a generator seeded by the case and then moved, so every file sees the same
numbers."""
import zlib

import numpy as np
import torch

import edge_checks as K
from edge_checks import C_BOUND, U, Out, bits_equal  # noqa: F401  (re-exported to the test files)

# ------------------------------------------------------------------------------------------------------- representation
# The representation is no plain sum (exponentials, a quotient, max / min, a square root, a norm), so it has no (L, A)
# bound; its bars are MEASURED: tests/test_mfv_ref_cpu.py::test_fp32_representation evaluates the definition
# (mfv_ref.get_3dmfv) in fp32 on every case's inputs and prints max-abs and relative-RMS error against float64.  Measured
# there (torch CPU, fp32), per case (B, N, K):
#   (1, 1, 8)       max-abs 7.66e-08  rel RMS 6.96e-08      (2, 7, 8)       max-abs 3.58e-07  rel RMS 1.43e-07
#   (3, 65, 27)     max-abs 3.47e-07  rel RMS 1.08e-07      (2, 300, 125)   max-abs 1.27e-07  rel RMS 1.03e-07
#   (1, 1025, 512)  max-abs 9.33e-08  rel RMS 8.74e-08      (2, 100, 10)    max-abs 1.28e-07  rel RMS 8.90e-08
# The GPU bar is FOUR times the worst of each; the factor covers the hardware exponential and the chunked reduction order.
# (The kernel itself, on an MI355X: worst max-abs 1.38e-06 at (2, 7, 8), worst relative RMS 2.54e-07 at the same case; the
# other five cases stay below 5.7e-07 and 2.4e-07.)
FV_MAXABS_FP32_WORST = 3.58e-7
FV_RMS_FP32_WORST = 1.43e-7
FV_MAXABS_BAR = 4 * FV_MAXABS_FP32_WORST
FV_RMS_BAR = 4 * FV_RMS_FP32_WORST

# (B, N, K): one point; few points; one point past a wave; K no multiple of 64; one point past a chunk with the largest K;
# a non-cubic, non-uniform, anisotropic mixture
FV_CASES = [(1, 1, 8), (2, 7, 8), (3, 65, 27), (2, 300, 125), (1, 1025, 512), (2, 100, 10)]
FV_OUTSIDE = (2, 300, 125)       # every point scaled by 1.5 and shifted by 0.2: much of the cloud leaves the grid
FV_ON_MEAN = (3, 65, 27)         # point 0 of cloud 0 lies exactly on a mean
FV_UNSUPPORTED = [(1, 16, 513), (1, 16, 1024)]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def grid_gmm(n, variance=0.04):
    """the closed form of get_3d_grid_gmm, written out here: means (2 i + 1) / n - 1 per axis, first axis slowest"""
    ax = torch.tensor([(2 * i + 1) / n - 1.0 for i in range(n)], dtype=torch.float64)
    mu = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    k = n ** 3
    return torch.full((k,), 1.0 / k, dtype=torch.float64), mu, torch.full((k, 3), float(np.sqrt(variance)), dtype=torch.float64)


def fv_inputs(case, device="cpu"):
    """points (B,N,3) fp32 inside the unit ball (a cloud normalised like the trainer's), w, mu, sigma fp32"""
    b, n, k = case
    g_ = gen("fv", case)
    pts = torch.randn(b, n, 3, generator=g_)
    pts = pts / pts.norm(dim=-1, keepdim=True) * torch.rand(b, n, 1, generator=g_) ** (1.0 / 3.0)
    root = round(k ** (1.0 / 3.0))
    if root ** 3 == k:
        w, mu, sigma = grid_gmm(root)
    else:
        w = 0.5 + torch.rand(k, generator=g_, dtype=torch.float64)
        w = w / w.sum()
        mu = 1.6 * torch.rand(k, 3, generator=g_, dtype=torch.float64) - 0.8
        sigma = 0.15 + 0.25 * torch.rand(k, 3, generator=g_, dtype=torch.float64)
    if case == FV_OUTSIDE:
        pts = pts * 1.5 + 0.2
    w, mu, sigma = w.float(), mu.float(), sigma.float()
    if case == FV_ON_MEAN:
        pts[0, 0] = mu[k // 2]
    return tuple(t.to(device).contiguous() for t in (pts, w, mu, sigma))


def fv_errors(out, ref64):
    """(max-abs, relative RMS) of a representation against the float64 definition"""
    err = (out.double() - ref64).abs()
    return err.max().item(), ((err ** 2).mean().sqrt() / (ref64 ** 2).mean().sqrt()).item()


# ---------------------------------------------------------------------------------------------------------- convolution
# Relative RMS against float64 of a SEQUENTIAL fp32 evaluation of each definition on the inputs below
# (tests/test_mfv_ref_cpu.py::test_fp32_conv prints these; largest per entry point over CONV_CASES):
#   conv3d_fwd y 2.76e-06 (1, 5, 5, 512, 256: 64 001 terms)      conv3d_dgrad dx 1.93e-06 (1, 5, 5, 512, 256: 32 000 terms)
#   conv3d_wgrad dw 1.11e-06, db 1.37e-06 (65, 5, 3, 64, 32: 8125 rows)
# The relative-RMS bar is twice the largest value: the rule tests/spider_checks.py:26-30 states (the factor of two leaves
# room for the chunked order of the MFMA accumulation and of the split reduction).  The per-element bound is
# edge_checks.check_sum's, unchanged.
RMS_FP32_SEQUENTIAL_WORST = 2.76e-6
RMS_BAR = 2 * RMS_FP32_SEQUENTIAL_WORST

# ((B, R, k, Cin, Cout), weight-gradient splits the launcher takes): the issue's seven cases, then one case per remaining
# split count (2 by the workgroup cap of a 500-workgroup grid, 8 by the step cap)
CONV_CASES = [
    ((1, 3, 5, 64, 32), 1),        # kernel wider than the grid; 27 rows: one 64-row step, so one split, direct store
    ((3, 3, 3, 64, 32), 2),        # a few clouds on the small grid; 81 rows: two steps
    ((65, 5, 3, 64, 32), 16),      # one row past a tile at every voxel
    ((2, 5, 5, 128, 64), 4),       # 5^3 kernel on the 5^3 grid, middle widths
    ((4, 8, 3, 128, 64), 16),      # the 8^3 grid
    ((2, 4, 5, 256, 128), 1),      # the 4^3 grid, 5^3 kernel; 1000 workgroups: one split
    ((1, 5, 5, 512, 256), 1),      # widest layer
    ((2, 3, 5, 128, 128), 1),      # Cout = Cin (outside the model, inside multiples of 16); 54 rows: one step
    ((5, 3, 5, 128, 128), 2),      # 500 workgroups: doubled once
    ((8, 5, 5, 64, 32), 8),        # 125 workgroups, 16 steps: 8 splits
    ((3, 2, 5, 64, 32), 1),        # the 2^3 grid of the 27-Gaussian model: the taps at offset +-2 have no row at all
]
CONV_UNSUPPORTED = [(1, 9, 3, 64, 32), (1, 5, 7, 64, 32), (1, 5, 1, 64, 32), (1, 5, 3, 60, 32), (1, 5, 3, 64, 40),
                    (1, 5, 3, 1024, 32)]


def conv_id(case):
    return "b%d_r%d_k%d_c%d_o%d" % tuple(case[0] if isinstance(case[0], tuple) else case)


def conv_inputs(shape, device="cpu"):
    """x (B,R,R,R,Cin), w (k,k,k,Cin,Cout), bias, dy (B,R,R,R,Cout) in the LOGICAL layout; x, w and dy carry a per-channel
    offset of 0.25 .. 0.75 so that no sum cancels to zero"""
    b, r, k, cin, cout = shape
    g_ = gen("conv3d", shape)

    def off(m):
        return 0.25 + 0.5 * torch.rand(m, generator=g_)

    x = torch.randn(b, r, r, r, cin, generator=g_) + off(cin)
    w = (torch.randn(k, k, k, cin, cout, generator=g_) + off(cout)) / float(np.sqrt(k ** 3 * cin))
    bias = 0.1 * torch.randn(cout, generator=g_) + 0.05
    dy = torch.randn(b, r, r, r, cout, generator=g_) + off(cout)
    return tuple(t.to(device).contiguous() for t in (x, w, bias, dy))


def check_sum(out, triple, what, report=None, rms=True):
    """edge_checks.check_sum itself -- |out - ref| <= C (L + 4) 2^-24 A per element -- with this family's RMS bar.
    rms=False: the per-element bound alone (the CPU test that MEASURES the relative RMS the bar is derived from)"""
    prev, K.RMS_BAR = K.RMS_BAR, RMS_BAR if rms else float("inf")
    try:
        K.check_sum(out, triple, what, report=report)
    finally:
        K.RMS_BAR = prev


# -------------------------------------------------------------------------------------------------------------- classifier
def randomise(net, seed):
    """non-trivial BN scales, offsets and moving statistics, and biases, for a freshly built model"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in list(net.named_parameters()) + list(net.named_buffers()):
            if name.endswith("gamma"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))
            elif name.endswith("beta") or name.endswith("biases"):
                p.copy_((0.2 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("moving_mean"):
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
            elif name.endswith("moving_variance"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))
