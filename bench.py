#!/usr/bin/env python3
"""Throughput harness for the hot path: PointNet++ SSG (BASELINE config 2), forward + backward + Adam,
point-clouds/sec on synthetic B x 2048 x 3 clouds resident in HBM.

  python bench.py --gpus N --steps K --warmup W

N > 1: one rank per GPU over RCCL.  Under `python -m torch.distributed.run ... bench.py --gpus N` the ranks are
already there (RANK / WORLD_SIZE in the environment); started bare (`python bench.py --gpus N`) the script
launches the N ranks itself through torch.distributed.run on 127.0.0.1.  Either way the run FAILS if the world
size it ends up with is not --gpus.

A "step" = one training step of `pointnet2_cls_ssg` on one batch of 256 clouds per GPU (weak scaling):
geometry (FPS / ball query / grouping) -> shared MLPs + BN + max-pool -> FC head -> loss -> backward ->
flat-bucket gradient all-reduce (RCCL) -> TF-Adam update.  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scanobjectnn_amd import _lib, dist as D  # noqa: E402
from scanobjectnn_amd import train_util as TU  # noqa: E402
from scanobjectnn_amd.graph import Model  # noqa: E402
from scanobjectnn_amd.synth import synth_clouds, synth_labels, synth_masks  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
F32_PEAK_TFLOPS = 157.3   # f32 vector == f32-input MFMA peak
BOOST_MHZ = 2400.0         # the clock the peaks below are quoted at
BF16_PEAK_TFLOPS = 2516.6  # dense bf16 MFMA peak (16 x the f32-input rate, MI355X_MICROARCH.md)
# kernels whose product runs on the bf16 matrix pipe with split operands: six bf16 products per
# fp32 product, so their matrix-pipe fraction is 6 x the algorithmic flops over the bf16 peak (= flops / (157.3 x 16 / 6))
SPLIT_OPERAND_KERNELS = ("pcops_mlp_gemm_fwd", "pcops_mlp_gemm_fwd_pool", "pcops_mlp_gemm_fwd_xyz",
                         "pcops_mlp_gemm_fwd_rows", "pcops_mlp_gemm_fwd_pool_rows", "pcops_mlp_gemm_fwd_xyz_rows")


class ClockPoller:
    """Shader clock and socket power of the busiest GPU while the timed region runs (rank 0; a host thread reading the
    amdgpu hwmon files at ~100 Hz, rocm-smi as the fallback).  Context for `roofline.frac`, which is priced against the
    peak at the part's boost clock: dense bf16 matrix work makes the chip clock down."""

    def __init__(self):
        import glob
        import threading
        self.freq = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"))
        # THIS process's GPU, by PCI address: the pool's nodes carry eight GPUs and the other seven are other tenants' -- "the
        # busiest GPU of the node" (rounds 4 to 6 until this fix) can be a neighbour's (profiles/r06_box_probe.txt)
        self.mine = None
        try:
            pr = torch.cuda.get_device_properties(torch.cuda.current_device())
            addr = "%04x:%02x:%02x.0" % (int(getattr(pr, "pci_domain_id", 0)), int(pr.pci_bus_id), int(pr.pci_device_id))
            mine = [f for f in self.freq if os.path.basename(os.path.realpath(f.split("/hwmon/")[0])) == addr]
            if mine:
                self.freq, self.mine = mine, addr
        except Exception:
            pass
        self.samples, self.stop_flag, self.source = [], False, None
        self.thread = threading.Thread(target=self._run, daemon=True)

    def _read_sysfs(self):
        best = None
        for f in self.freq:
            try:
                mhz = int(open(f).read()) / 1e6
                d = os.path.dirname(f)
                pw = None
                for name in ("power1_average", "power1_input"):
                    if os.path.exists(os.path.join(d, name)):
                        pw = int(open(os.path.join(d, name)).read()) / 1e6
                        break
                if pw is not None and (best is None or pw > best[1]):
                    best = (mhz, pw)
            except (OSError, ValueError):
                continue
        return best

    def _read_smi(self):
        import re
        import subprocess
        out = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=5).stdout
        pw = [float(v) for v in re.findall(r"Power \(W\): ([\d.]+)", out)]
        ck = [int(v) for v in re.findall(r"sclk clock level: \d+: \((\d+)Mhz\)", out)]
        if not pw or len(pw) != len(ck):
            return None
        i = max(range(len(pw)), key=lambda j: pw[j])
        return (float(ck[i]), pw[i])

    def _run(self):
        reader = self._read_sysfs if self.freq and self._read_sysfs() else self._read_smi
        self.source = "amdgpu hwmon (freq1_input, power1_average), ~100 Hz" if reader == self._read_sysfs else "rocm-smi"
        self.source += (", device %s" % self.mine) if (self.mine and reader == self._read_sysfs) else \
            ", the busiest of the node's GPUs (device not identified: may be a neighbour's)"
        while not self.stop_flag:
            try:
                v = reader()
            except Exception:
                v = None
            if v:
                self.samples.append(v)
            if reader == self._read_sysfs:
                time.sleep(0.01)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *a):
        self.stop_flag = True
        self.thread.join(timeout=10)

    def summary(self):
        busy = [v for v in self.samples if v[1] > 500.0] or self.samples
        if not busy:
            return None
        ck, pw = sorted(v[0] for v in busy), sorted(v[1] for v in busy)
        return {"sclk_mhz": sum(ck) / len(ck), "power_w": sum(pw) / len(pw),
                "sclk_mhz_min_median_max": [ck[0], ck[len(ck) // 2], ck[-1]],
                "power_w_min_median_max": [pw[0], pw[len(pw) // 2], pw[-1]],
                "samples": len(busy), "source": self.source, "boost_mhz": BOOST_MHZ}


def _split_operands(d):
    """did this launch run on the bf16 matrix pipe with split operands?  The LIBRARY's own answer, read back right after
    the launch (pcops_last_launch_pipe, KernelTimer) -- not a mirror of ws_plan / wgrad_bf3_plan's rules"""
    return d["work_unit"] == "flop" and d.get("pipe_code") == 1


def _half_split(d):
    """the one-pass backward: its dW half on the fp32 pipe, its dX half on the bf16 pipe with split operands
    (bwd_fused_kernel<..., DX3>)"""
    return d["work_unit"] == "flop" and d.get("pipe_code") == 2


def _mfma_frac(d):
    """fraction of the matrix pipe's peak a kernel's ALGORITHMIC flops stand for on the pipe it runs on"""
    if d["work_unit"] != "flop":
        return 0.0
    if _split_operands(d):
        return 6.0 * d["gwork_s"] / 1e3 / BF16_PEAK_TFLOPS
    return d["gwork_s"] / 1e3 / F32_PEAK_TFLOPS


def _pipe_busy(d):
    """share of the launch the matrix pipe is busy at its nominal rate: the fp32 part of the flops at the fp32 rate, the
    split-operand part six-fold at the bf16 rate"""
    if d["work_unit"] != "flop":
        return None
    tf = d["gwork_s"] / 1e3
    if _split_operands(d):
        return 6.0 * tf / BF16_PEAK_TFLOPS
    if _half_split(d):
        return 0.5 * tf / F32_PEAK_TFLOPS + 0.5 * 6.0 * tf / BF16_PEAK_TFLOPS
    return tf / F32_PEAK_TFLOPS
MEASURED_F32_MFMA_TFLOPS = 155.0   # tools/ubench/mfma_peak.hip on this chip (operands in registers, 2.37 GHz)
MEASURED_HBM_GBS = 6290.0          # MI355X_MICROARCH.md: float4 copy, 79 % of spec
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9    # 256 CUs x 4 SIMD-32 at 2.4 GHz = 78.6 T fp32 lane-ops/s
QBP_VALU_OPS_PER_PAIR = 9          # 3 sub, 3 mul, 2 add (uncontracted) + 1 compare

MODELS = {
    "pointnet2_cls_ssg": ("scanobjectnn_amd.pointnet2.pointnet2_cls_ssg", False, 256, 2048),
    "pointnet2_cls_bga": ("scanobjectnn_amd.pointnet2.pointnet2_cls_bga", True, 128, 2048),
    "pointnet2_cls_msg": ("scanobjectnn_amd.pointnet2.pointnet2_cls_msg", False, 256, 4096),
    "dgcnn": ("scanobjectnn_amd.dgcnn.dgcnn", False, 256, 2048),
    "dgcnn_bga": ("scanobjectnn_amd.dgcnn.dgcnn_bga", True, 128, 2048),
}


# ---- algorithmic bytes / flops per launch of each pcops kernel (SURVEY.md §8d formulas) --------
def _algo(name, a):
    """returns (bytes, work, work_unit) for one launch given the C-ABI argument tuple; `work` = flops for the
    MFMA kernels, pair tests for the search kernels"""
    if name == "pcops_query_ball_point":
        b, n, m, _r, s = a[:5]
        return b * (12 * n + 12 * m + 4 * m * s + 4 * m), b * m * n, "pairs"
    if name == "pcops_query_ball_point_multi":
        b, n, m = a[:3]
        return b * (12 * n + 12 * m), b * m * n, "pairs"
    if name == "pcops_farthest_point_sample":
        b, n, m = a[:3]
        return b * (12 * n + 4 * m), b * (m - 1) * n, "pairs"
    if name == "pcops_gather_point":
        b, n, m = a[:3]
        return b * (16 * m + 12 * m), 0, ""
    if name == "pcops_gather_point_grad":
        b, n, m = a[:3]
        return b * (16 * m + 12 * n), 0, ""
    if name in ("pcops_group_point", "pcops_group_point_grad"):
        b, n, c, m, s = a[:5]
        return b * (4 * n * c + 4 * m * s + 4 * m * s * c), 0, ""
    if name == "pcops_three_nn":
        b, n, m = a[:3]
        return b * (12 * n + 12 * m + 24 * n), b * n * m, "pairs"
    if name in ("pcops_three_interpolate", "pcops_three_interpolate_grad"):
        b, m, c, n = a[:4] if name == "pcops_three_interpolate" else (a[0], a[3], a[2], a[1])
        return b * (4 * m * c + 24 * n + 4 * n * c), 0, ""
    if name in ("pcops_knn_graph", "pcops_knn_graph_seeded"):      # (seeded: + the hint's k indices per query)
        b, n, c, k = a[:4]
        # counted in PAIR TESTS, like the other search kernels: the distances of the 64-channel graphs run as fp16 MFMAs that
        # keep the matrix pipe busy 3.5 % of the launch, and what binds is instruction issue in the selection (574 k
        # wave-instructions per SIMD and launch, profiles/r04_pmc_insts_dgcnn.txt) -- pricing 2 n^2 c flops against the fp32
        # matrix peak (rounds 2-4) named a bound the kernel does not have
        return b * (4 * n * c + 4 * n * k * (2 if name.endswith("seeded") else 1)), b * n * n, "pairs"
    if name in ("pcops_edge_feature", "pcops_edge_feature_grad"):
        b, n, c, k = a[:4]
        return b * (4 * n * c + 4 * n * k + 8 * n * k * c), 0, ""
    # ---- shared-MLP kernels: activations only (weights / per-channel vectors are negligible)
    if name == "pcops_mlp_gemm_fwd":          # Y[M,N] = f(X)[M,K] W
        M, K, N = a[:3]
        return 4 * (M * K + M * N), 2 * M * K * N, "flop"
    if name == "pcops_mlp_gemm_fwd_xyz":      # operand rebuilt from 16 bytes per row
        M, K, N = a[:3]
        return 4 * (4 * M + M * N), 2 * M * K * N, "flop"
    if name == "pcops_mlp_gemm_dgrad_xyz":    # reads G?, Y (K wide) + 16 bytes per row; writes Gprev
        M, K, Nout = a[:3]
        return 4 * ((1 if a[3] is None else 2) * M * K + 4 * M + (M * Nout if a[18] is not None else 0)), 2 * M * K * Nout, "flop"
    if name == "pcops_mlp_wgrad_xyz":         # reads 16 bytes per row + G?, Y
        M, K, N = a[:3]
        return 4 * (4 * M + (1 if a[7] is None else 2) * M * N), 2 * M * K * N, "flop"
    if name == "pcops_mlp_gemm_fwd_pool":     # + raw extrema per group
        M, K, N, S = a[:4]
        return 4 * (M * K + M * N) + 5 * (M // S) * N, 2 * M * K * N, "flop"
    if name == "pcops_mlp_pool_select":
        G, C = a[:2]
        return 8 * G * C, 0, ""
    if name == "pcops_mlp_gemm_dgrad":        # Gprev[M,Nout] = mask . (dY[M,K] Wt); reads G?,Y (K wide), Yprev (Nout)
        M, K, Nout = a[:3]
        reads = (1 if a[3] is None else 2) * M * K + (M * Nout if a[14] is not None else 0)
        return 4 * (reads + M * Nout), 2 * M * K * Nout, "flop"
    if name == "pcops_mlp_wgrad":             # dW[K,N] = A[M,K]^T dY[M,N]; reads X, G?, Y
        M, K, N = a[:3]
        return 4 * (M * K + (1 if a[7] is None else 2) * M * N), 2 * M * K * N, "flop"
    if name == "pcops_mlp_bwd_fused":         # data + weight gradient in one pass: reads Yprev (K), G?, Y (N); writes Gprev (K)
        M, K, N = a[:3]
        return 4 * (2 * M * K + (1 if a[6] is None else 2) * M * N), 4 * M * K * N, "flop"
    if name == "pcops_mlp_bwd_fused_gw":      # pooled form with the weight gradient as a Gram matrix: same bytes; the flops
        M, K, N = a[:3]                       # EXECUTED are 2 M K (N + K) (+ 2 K N per arg row) -- the algorithmic ones priced
        return 4 * (2 * M * K + M * N), 4 * M * K * N, "flop"
    if name in ("pcops_mlp_bwd_fused_edge", "pcops_mlp_bwd_fused_edge_gw"):
        # ... above a first EdgeConv layer without input gradient: Yprev, Y and 32 B of edge channels per row in, NO Gprev
        # (its E^T Gprev is reduced in the kernel)
        M, K, N = a[:3]
        return 4 * (M * K + M * N + 8 * M), 4 * M * K * N, "flop"
    if name == "pcops_cloud_bias_fwd":        # Y = Q + Ctr[cloud]: Q in, Y out
        rows, rpg, c = a[:3]
        return 8 * rows * c, 0, ""
    if name == "pcops_cloud_bias_bwd":        # G, Y in; dQ out
        rows, rpg, c = a[:3]
        return 4 * rows * c * (3 if a[8] is not None else 2), 0, ""
    if name == "pcops_edge_first_wgrad":      # E^T Gm: one pass over the masked gradient (b m s rows of c)
        b, n, m, s_, c = a[:5]
        return 4 * b * m * s_ * (c + 1), 12 * b * m * s_ * c, "flop(VALU)"
    if name == "pcops_edge_first_moments":    # idx + the gathered cloud in; (optionally) the 32-byte edge rows out
        b, n, m, s_ = a[:4]
        return b * m * s_ * (4 + (32 if a[7] is not None else 0)), 0, ""
    if name == "pcops_mlp_bwd_fused_xyz":     # ... over the xyz form: 16 bytes per row instead of Yprev, no Gprev
        M, K, N = a[:3]
        return 4 * (4 * M + (1 if a[7] is None else 2) * M * N), 4 * M * K * N, "flop"
    # ---- algebraic backward of a pooled top layer (pcops.h): K x K products + the arg-max rows
    if name == "pcops_mlp_gemm_dgrad_top":    # Gprev[M,Kp] = mask . (X Mq + addend rows + v): reads X, writes Gprev
        M, Kp = a[:2]
        return 4 * (2 * M * Kp), 2 * M * Kp * Kp, "flop"
    if name == "pcops_mlp_gram":              # X^T X: one pass over X; symmetric -- the work is the upper triangle
        M, Kp = a[:2]
        return 4 * M * Kp, M * Kp * (Kp + 1), "flop"
    if name == "pcops_mlp_pool_top_addend":   # per (group, channel) 9 bytes in, a Kp-wide weight row through L2, compact rows out
        M, Kp, N, S = a[:4]
        return (M // S) * N * 9 + 4 * (M // S) * min(S, N) * Kp + 4 * M, 2 * (M // S) * N * Kp, "flop(VALU)"
    if name == "pcops_mlp_pool_top_wsparse":  # per (group, channel) 9 bytes in + a Kp-wide activation row
        M, Kp, N, S = a[:4]
        return (M // S) * N * (9 + 4 * Kp), 2 * (M // S) * N * Kp, "flop(VALU)"
    if name in ("pcops_small_gemm", "pcops_small_gemm_ex", "pcops_small_gemm_colsum"):
        M, K, N = a[:3]
        return 4 * (M * K + K * N + M * N), 2 * M * K * N, "flop"
    if name == "pcops_small_gemm_pair":       # two products in one launch
        M0, K0, N0, M1, K1, N1 = a[:6]
        return 4 * (M0 * K0 + K0 * N0 + M0 * N0 + M1 * K1 + K1 * N1 + M1 * N1), 2 * (M0 * K0 * N0 + M1 * K1 * N1), "flop"
    if name == "pcops_mlp_pool_top_prep":     # W read once; W^T and W diag(q) written (the row products re-read W through L2)
        Kp, N = a[:2]
        return 4 * 3 * Kp * N, 0, ""
    if name == "pcops_mlp_pool_top_finish":   # dW read and written, Ssp read, W read for the column sums
        Kp, N = a[:2]
        return 4 * 4 * Kp * N, 0, ""
    if name == "pcops_softmax_ce":            # logits in, gradient out
        R, C = a[:2]
        return 4 * 2 * R * C + 4 * R, 0, ""
    if name == "pcops_mlp_pool_bwd_stats_sum":    # both pieces and ysel read, the contiguous sum written
        G, C = a[:2]
        return 4 * G * C * (3 + (1 if a[4] is not None else 0)), 0, ""
    if name == "pcops_mlp_dy_apply":          # G and Y read, dY written
        M, N = a[:2]
        return 4 * 3 * M * N, 0, ""
    if name == "pcops_mlp_bn_relu_maxpool":
        G, S, C = a[:3]
        return 4 * G * S * C + 5 * G * C, 0, ""
    if name == "pcops_mlp_bn_relu_maxpool_rows":      # (rows computed, C): the max over compacted groups re-reads Y once
        R, C = a[:2]
        return 4 * R * C, 0, ""
    if name == "pcops_mlp_pool_combine_rows":         # (rows computed, C): one partial per 16-row block, 5 bytes each
        R, C = a[:2]
        return 5 * (R // 16) * C, 0, ""
    if name == "pcops_mlp_bn_relu_apply":
        R, C = a[:2]
        return 8 * R * C, 0, ""
    if name == "pcops_mlp_relu_mask_stats":
        R, C = a[:2]
        return 12 * R * C, 0, ""
    if name == "pcops_mlp_pool_bwd_stats":
        G, C = a[:2]
        return 8 * G * C, 0, ""
    if name in ("pcops_edge_pool_fwd", "pcops_edge_pool_fwd_ld"):     # Q, Ctr, idx read once (algorithmically); SQ, qsel, arg written
        b, n, m, s_, c = a[:5]
        return 4 * (b * n * c + b * m * c + b * m * s_) + 9 * b * m * c, 0, ""
    if name in ("pcops_edge_pool_bwd", "pcops_edge_pool_bwd_ld"):     # + gpool, ysel, SQ, arg read; dQ, dCtr written
        b, n, m, s_, c = a[:5]
        return 4 * (2 * b * n * c + 2 * b * m * c + b * m * s_) + 13 * b * m * c, 0, ""
    if name in ("pcops_edge_pool_out", "pcops_edge_pool_out_ld", "pcops_edge_pool_out_ld2"):
        # qsel, Ctr in; out + ysel out (+ the second copy into the concatenation's column block)
        groups, c = a[:2]
        return 4 * groups * c * (5 if (name.endswith("ld2") and a[9] is not None) else 4), 0, ""
    if name == "pcops_sa_gather_fwd_ld":      # Y = Q[idx] + Ctr stored (b m s c); Q, Ctr (b n c) and idx read once
        b, n, m, s_, c = a[:5]
        return 4 * (b * m * s_ * c + 2 * b * n * c + b * m * s_), 0, ""
    if name == "pcops_sa_scatter_bwd_ld":     # G read for dCtr (streamed) and for dQ (gathered): 2 x (b m s c); dQ, dCtr out
        b, n, m, s_, c = a[:5]
        return 4 * (2 * b * m * s_ * c + b * m * s_ + 4 * b * n * c), 0, ""
    if name == "pcops_scatter_rows_sorted":   # src rows gathered once, idx (+ w), out written (ordered owner walk)
        b, rows, ndst, c, div = a[:5]
        return 4 * (b * (rows // max(div, 1)) * c + b * rows * (2 if a[7] is not None else 1) + b * ndst * c), 0, ""
    if name in ("pcops_fc_bn_fwd", "pcops_fc_bn_bwd"):
        R, C = a[:2]
        return 4 * R * C * (2 if name.endswith("fwd") else 4), 0, ""
    if name == "pcops_sa_gather_fwd":         # Y (b,m,s,c) written once; Q read once (algorithmically), idx
        b, n, m, s, c = a[:5]
        wr = (b * m * s * c if a[12] is not None else 0) + (4 * b * m * s if a[13] is not None else 0)
        return 4 * (wr + (b * n * c if a[5] is not None else 0) + b * m * s), 0, ""
    if name == "pcops_sa_scatter_bwd":        # reads G?,Y (b,m,s,c), idx; writes dQ (b,n,c)
        b, n, m, s, c = a[:5]
        return 4 * ((1 if a[5] is None else 2) * b * m * s * c + b * m * s + (b * n * c if a[17] is not None else 0)), 0, ""
    return 0, 0, ""


_NSHAPE = {"pcops_query_ball_point": 5, "pcops_query_ball_point_multi": 4, "pcops_group_point": 5,
           "pcops_group_point_grad": 5, "pcops_three_interpolate": 4, "pcops_three_interpolate_grad": 4,
           "pcops_knn_graph": 4, "pcops_knn_graph_seeded": 4, "pcops_edge_feature": 4, "pcops_edge_feature_grad": 4,
           "pcops_selection_sort": 4, "pcops_pairwise_distance": 3, "pcops_knn_topk": 3,
           "pcops_sa_gather_fwd": 5, "pcops_sa_scatter_bwd": 5, "pcops_mlp_bn_finalize": 3,
           "pcops_mlp_bn_bwd_coeffs": 3, "pcops_mlp_bn_relu_apply": 2, "pcops_mlp_relu_mask_stats": 2,
           "pcops_mlp_transpose": 2, "pcops_mlp_bn_eval_coeffs": 1, "pcops_mlp_gemm_fwd_pool": 4,
           "pcops_mlp_pool_select": 2, "pcops_mlp_pool_bwd_stats": 2, "pcops_xyz_first_layer_grads": 1,
           "pcops_edge_pool_fwd": 5, "pcops_edge_pool_bwd": 5, "pcops_edge_pool_out": 2,
           "pcops_mlp_bn_relu_maxpool_rows": 2, "pcops_mlp_pool_combine_rows": 2,
           "pcops_mlp_gemm_dgrad_top": 2, "pcops_mlp_gram": 2, "pcops_mlp_pool_top_addend": 4,
           "pcops_mlp_pool_top_wsparse": 4, "pcops_scatter_rows_sorted": 5, "pcops_edge_feature_grad_central": 4,
           "pcops_edge_pool_fwd_ld": 5, "pcops_edge_pool_bwd_ld": 5, "pcops_edge_pool_out_ld": 2, "pcops_edge_pool_out_ld2": 2,
           "pcops_sa_gather_fwd_ld": 5, "pcops_sa_scatter_bwd_ld": 5, "pcops_fc_bn_fwd": 2, "pcops_fc_bn_bwd": 2,
           "pcops_small_gemm": 3, "pcops_small_gemm_ex": 3, "pcops_small_gemm_colsum": 3, "pcops_mlp_pool_top_prep": 2,
           "pcops_mlp_pool_top_finish": 3, "pcops_softmax_ce": 2, "pcops_mlp_dy_apply": 2,
           "pcops_mlp_pool_bwd_stats_sum": 2, "pcops_small_gemm_pair": 6}


class KernelTimer:
    """HIP-event timing of every libpcops launch on the stream it is launched on (torch's current
    stream: `_lib.call` passes torch.cuda.current_stream() to the C ABI, and torch.cuda.Event.record()
    records on that same stream)."""

    def __init__(self, only=None):
        self.records = []     # (name, args, start_event, end_event)
        self._open = None
        self._rows = {}       # id -> _lib.Rows of the compacted stacks seen (kept alive until the summary)
        # only = (kernel, shape) of ONE table row: nothing else is bracketed (two event records per launch of ~160
        # launches cost ~0.4 ms of a 13 ms step; the timed region only carries the dominant kernel's events)
        self.only = None
        if only is not None:
            self.only = (only[0], tuple(x for x in only[1] if x != "compacted"))

    def _rows_computed(self, rows):
        """rows a compacted stack really computed (a 4-byte device -> host copy, after the timed region)"""
        return rows.num_rows()

    def __call__(self, name, phase, args):
        if name in ("pcops_mlp_bn_relu_maxpool_rows", "pcops_mlp_pool_combine_rows"):
            # (G, C, ...) with the pcops_rows_t* in the middle: keep the name, shape = (G, C)
            ref = args[5] if name == "pcops_mlp_bn_relu_maxpool_rows" else args[7]
            args = args[:2]
            owner = _lib.Rows.by_struct.get(id(ref._obj))
            if owner is not None:
                self._rows[id(owner)] = owner
                args = args + (("rows", id(owner)),)
        elif name == "pcops_mlp_gemm_fwd_pool_rows":
            # per-block pooled epilogue on compacted rows: accounted like the plain forward GEMM (+ the block partials)
            ref, args, name = args[-1], args[:3], "pcops_mlp_gemm_fwd"
            owner = _lib.Rows.by_struct.get(id(ref._obj))
            if owner is not None:
                self._rows[id(owner)] = owner
                args = args + ("pool", ("rows", id(owner)))
        elif name.endswith("_rows"):
            # compacted-row entry points (pcops.h): same argument list + a pcops_rows_t*; NULL = the plain entry point
            ref, args, name = args[-1], args[:-1], name[:-5]
            if ref is not None:
                owner = _lib.Rows.by_struct.get(id(ref._obj))
                if owner is not None:
                    self._rows[id(owner)] = owner           # kept alive until the summary reads its row count
                    args = args + (("rows", id(owner)),)
        if self.only is not None:
            n = _NSHAPE.get(name, 3)
            if name != self.only[0] or tuple(args[:n]) != self.only[1][:n]:
                return
        if phase == "pre":
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._open = ev
        else:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.records.append((name, args, self._open, ev, int(_lib.load().pcops_last_launch_pipe())))

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        frac_cache = {}
        for name, args, s, e, pipe in self.records:
            ms = s.elapsed_time(e)
            compacted = None
            if args and isinstance(args[-1], tuple) and args[-1][0] == "rows":
                rid, args = args[-1][1], args[:-1]
                if rid not in frac_cache:
                    frac_cache[rid] = self._rows_computed(self._rows[rid])
                compacted = frac_cache[rid]
            full_args = args
            if compacted is not None and name.startswith("pcops_mlp_"):
                args = (compacted,) + tuple(args[1:])          # the rows the kernel really walks
            by, work, unit = _algo(name, args)
            if compacted is not None and name.startswith("pcops_sa_"):
                b_, n_, m_, s_ = full_args[:4]
                scale = compacted / float(b_ * m_ * s_)
                by = int(by * scale)                           # dominated by the (rows, c) activations
            args = full_args
            key = (name,) + tuple(args[:_NSHAPE.get(name, 3)]) + (("compacted",) if compacted is not None else ())
            d = agg.setdefault(key, {"kernel": name, "shape": list(key[1:]), "launches": 0, "ms": 0.0,
                                     "bytes": 0, "work": 0, "work_unit": unit})
            d["launches"] += 1
            d["pipe_code"] = pipe if unit == "flop" else 0     # the matrix pipe the library took for this launch
            d["ms"] += ms
            d["bytes"] += by          # per-launch averages below: compacted row counts vary from step to step
            d["work"] += work
            if compacted is not None:
                d["rows_computed"] = d.get("rows_computed", 0) + compacted
        out = []
        for d in agg.values():
            avg_ms = d["ms"] / d["launches"]
            d["bytes"] /= d["launches"]
            d["work"] /= d["launches"]
            if "rows_computed" in d:
                d["rows_computed"] /= d["launches"]
            d["avg_us"] = avg_ms * 1e3
            d["gbs"] = d["bytes"] / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            d["gwork_s"] = d["work"] / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            out.append(d)
        out.sort(key=lambda d: -d["ms"])
        return out


def _measured_traffic(dom):
    """HBM bytes per launch of the dominant kernel from the committed PMC passes (profiles/*_pmc_traffic.json:
    FETCH_SIZE doubled per MI355X_MICROARCH.md + WRITE_SIZE, collected by tools/collect_traffic.sh), or None."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")), reverse=True):
        try:
            table = json.load(open(f))
        except Exception:
            continue
        key = "%s%s" % (dom["kernel"], tuple(dom["shape"]))
        if key in table:
            _measured_traffic.source = os.path.relpath(f, ROOT)
            return table[key]
    return None


_measured_traffic.source = None


def _ball_query_fractions(x, kernels):
    """SA1 ball query of the SSG config on the bench's own clouds: pair tests executed, fp32-VALU fraction and HBM
    fraction.  The kernel keeps a cloud in registers and tests every query against all of it (one bit per hit, no
    early exit -- csrc/grouping.hip), so executed pairs = b*m*n; it is bound by instruction issue (9 VALU lane-ops per
    pair test at best), not by HBM: both fractions are reported, as SURVEY.md section 8d asks."""
    from scanobjectnn_amd.pointnet2 import tf_grouping, tf_sampling
    out = {}
    for d in kernels:
        if d["kernel"] != "pcops_query_ball_point":
            continue
        b, n, m, r, s = d["shape"][:5]
        if (b, n) != (x.shape[0], x.shape[1]):
            continue        # only the level whose inputs can be rebuilt here (SA1)
        with torch.no_grad():
            q = tf_sampling.gather_point(x, tf_sampling.farthest_point_sample(m, x))
            idx, cnt = tf_grouping.query_ball_point(float(r), int(s), x, q)
            executed = b * m * n
        t = d["avg_us"] * 1e-6
        out = {"shape": d["shape"], "avg_us": d["avg_us"], "pairs_nominal": b * m * n, "pairs_executed": executed,
               "pair_tests_per_s": executed / t,
               "valu_frac": executed * QBP_VALU_OPS_PER_PAIR / t / VALU_LANE_OPS_PER_S,
               "hbm_frac": d["bytes"] / t / 1e9 / HBM_PEAK_GBS,
               "bound": "fp32 VALU (brute-force scan: %d lane-ops per pair test)" % QBP_VALU_OPS_PER_PAIR,
               "padding_frac": float(1.0 - cnt.float().mean().item() / s)}
    return out


def cpu_baseline(model_name, n_points, seconds_budget=15.0):
    """The CPU restatement (oracle/ref_models.py + the C oracle for the geometry) of the SAME step
    (forward + backward, training-mode BN, no optimiser), timed on the host cores of this box."""
    from oracle import ref_models as R
    import importlib
    modpath, has_mask, _, _ = MODELS[model_name]
    mod = importlib.import_module(modpath)
    ref_fn = getattr(R, model_name)
    cores = min(32, os.cpu_count() or 1)   # more threads only oversubscribe these small GEMMs
    torch.set_num_threads(cores)
    bs = 4
    c = synth_clouds(bs, n_points, seed=99)
    # variables: build the product graph once on the GPU to get identically-shaped weights
    net = Model(mod.get_model, device="cuda:0", seed=0).build(torch.from_numpy(c[:2]).cuda())
    P = {k: v.requires_grad_(v.is_floating_point()) for k, v in R.params_from_state_dict(net.state_dict()).items()}
    y = torch.from_numpy(synth_labels(bs)).long()
    x = torch.from_numpy(c)
    done, t0 = 0, time.perf_counter()
    while True:
        out = ref_fn(x, P, True)
        logits = out[0] if isinstance(out, tuple) else out
        loss = torch.nn.functional.cross_entropy(logits, y)
        if isinstance(out, tuple):
            loss = loss + out[1].square().mean()
        loss.backward()
        done += bs
        el = time.perf_counter() - t0
        if el > seconds_budget or done >= 1024:
            break
    return {"value": done / el, "unit": "clouds/s", "cores": cores, "kind": "port",
            "sample": "%d clouds of %d pts, %s forward+backward (train-mode BN), oracle/ref_models.py "
                      "(C oracle geometry, 1 thread) + torch-CPU fp32 algebra (%d threads), %.1f s"
                      % (done, n_points, model_name, cores, el)}


def cpu_ops_baseline(seconds_budget=6.0):
    """the op-level CPU figures.  The reference's own CPU twins (query_ball_point_cpu,
    group_point_cpu, group_point_grad_cpu, threenn_cpu, threeinterpolate_cpu, threeinterpolate_grad_cpu) at the
    reference's own bench sizes (tf_ops/grouping/test/query_ball_point.cpp:86-119: b=32 n=512 m=128 nsample=64 c=64
    r=0.1; 3d_interpolation/interpolate.cpp:132-169: b=32 n=512 m=128 c=64), timed (a) on one core as they are and
    (b) sharded by cloud over the host cores (one process per shard, no code change).  `kind` says what ran:
    "reference" = oracle/_ref (the reference sources compiled in the build container, prebuilt .so shipped),
    "port" = oracle/pcops_oracle.c (validated bit-exact against them by tests/test_oracle_golden.py)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as O
    kind = "reference" if O.have_ref() else "port"
    rng = np.random.default_rng(5)
    b, n, m, s, c, r = 32, 512, 128, 64, 64, 0.1
    xyz1 = rng.random((b, n, 3), dtype=np.float32)
    xyz2 = rng.random((b, m, 3), dtype=np.float32)
    pts = rng.random((b, n, c), dtype=np.float32)
    idx = O.query_ball_point(r, s, xyz1, xyz2)[0]
    gout = rng.random((b, m, s, c), dtype=np.float32)
    w = rng.random((b, n, 3), dtype=np.float32)
    i3 = rng.integers(0, m, (b, n, 3)).astype(np.int32)
    p2 = rng.random((b, m, c), dtype=np.float32)
    g2 = rng.random((b, n, c), dtype=np.float32)
    R = kind == "reference"
    import threading
    tls = threading.local()

    def gp_out(sl):
        # group_point writes 67 MB per reference-size batch: one buffer per worker thread, touched once -- a fresh array
        # per call would measure the kernel's page-fault path (32 threads took 86 ms per batch against 4 ms on one core)
        nb = len(range(*sl.indices(b)))
        if getattr(tls, "gp", None) is None or tls.gp.shape[0] != nb:
            tls.gp = np.zeros((nb, m, s, c), np.float32)
        return tls.gp
    ops = {
        "query_ball_point": ((lambda sl: (O.ref_query_ball_point if R else (lambda *a: O.query_ball_point(*a)[0]))(r, s, xyz1[sl], xyz2[sl]))),
        "group_point": (lambda sl: (O.ref_group_point if R else O.group_point)(pts[sl], idx[sl], out=gp_out(sl))),
        "group_point_grad": (lambda sl: (O.ref_group_point_grad if R else O.group_point_grad)(pts[sl].shape, idx[sl], gout[sl])),
        "three_nn": (lambda sl: (O.ref_three_nn if R else O.three_nn)(xyz1[sl], xyz2[sl])),
        "three_interpolate": (lambda sl: (O.ref_three_interpolate if R else O.three_interpolate)(p2[sl], i3[sl], w[sl])),
        "three_interpolate_grad": (lambda sl: (O.ref_three_interpolate_grad if R else O.three_interpolate_grad)(p2[sl].shape, i3[sl], w[sl], g2[sl])),
    }
    cores = min(32, os.cpu_count() or 1)
    out = {}
    t_all = time.perf_counter()
    full = slice(0, b)
    for name, fn in ops.items():
        fn(slice(0, 1))
        t0 = time.perf_counter()
        reps = 0
        while True:
            fn(full)
            reps += 1
            if time.perf_counter() - t0 > seconds_budget / (2 * len(ops)) or reps >= 20:
                break
        one = (time.perf_counter() - t0) / reps
        # sharded over the host cores the way a data-parallel caller would, no code change in the functions: `cores`
        # PERSISTENT workers, each running whole reference-size batches (b clouds per call, i.e. 32 x cores clouds per
        # round) -- a call is milliseconds of C code outside the GIL, so the figure is the ops' and not the thread
        # pool's (round 2 split ONE 32-cloud batch into 32 single-cloud calls: 70 us of work per dispatch)
        k = max(1, int(min(20, (seconds_budget / (2 * len(ops))) / max(one, 1e-4))))
        with ThreadPoolExecutor(max_workers=cores) as ex:
            def worker(_):
                for _i in range(k):
                    fn(full)
            list(ex.map(worker, range(cores)))     # warm the pool (and the page cache of every worker's buffers)
            t0 = time.perf_counter()
            list(ex.map(worker, range(cores)))
            sharded = time.perf_counter() - t0
        per_batch = sharded / k                    # `cores` batches complete per this time
        out[name] = {"ms_1core": one * 1e3, "clouds_per_s_1core": b / one,
                     "ms_sharded": per_batch * 1e3, "clouds_per_s_sharded": b * cores / per_batch,
                     "speedup_sharded": (b * cores / per_batch) / (b / one)}
    return {"kind": kind, "cores_sharded": cores, "shape": {"b": b, "n": n, "m": m, "nsample": s, "c": c, "radius": r},
            "clouds_per_round_sharded": b * cores, "ops": out, "seconds": time.perf_counter() - t_all,
            "note": "sharded = `cores` persistent threads, each calling the C function on whole reference-size batches "
                    "(ms_sharded = time in which `cores` batches of b clouds complete); the C functions run outside the GIL"}


def side_model(name, dev, steps=10, warmup=3):
    """SURVEY.md section 8 / BASELINE.json configs[2..4] next to the metric: one short training run (fwd + bwd + TF-Adam,
    per-GPU batch of the config) of another in-scope model on the same kernels -> clouds/s, and its dominant kernel
    with the roofline fraction from a separate bracketed pass.  Never part of `value`."""
    import gc
    import importlib
    modpath, has_mask, B, N = MODELS[name]
    mod = importlib.import_module(modpath)
    x = torch.from_numpy(synth_clouds(B, N, seed=77)).to(dev)
    y = torch.from_numpy(synth_labels(B, seed=77)).to(dev)
    mask = torch.from_numpy(synth_masks(B, N, seed=77)).to(dev) if has_mask else None
    net = Model(mod.get_model, device=dev, seed=0).build(x[:2].contiguous())
    fp = TU.FlatParams(net)
    opt = TU.TFAdam(fp)
    st = {"step": 0}

    def step():
        fp.begin_step()
        out = net(x, is_training=True, bn_decay=TU.get_bn_decay(st["step"], B))
        loss = mod.get_loss(out[0], out[1], y, mask)[0] if has_mask else mod.get_loss(out[0], y, out[1])
        loss.backward()
        fp.collect()
        opt.step(TU.get_learning_rate(st["step"], B))
        st["step"] += 1

    for _ in range(warmup):
        step()
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    timer = KernelTimer(None)
    _lib._hooks.append(timer)
    try:
        for _ in range(3):
            step()
    finally:
        _lib._hooks.remove(timer)
    ks = timer.summary()
    res = {"clouds_per_s": B * steps / el, "ms_per_step": el / steps * 1e3, "batch": B, "num_point": N, "steps": steps,
           "train_step": "fwd+bwd+Adam", "launches_per_step": sum(d["launches"] for d in ks) / 3.0}
    if ks:
        d = ks[0]
        hbm = d["gbs"] / HBM_PEAK_GBS
        mf = _mfma_frac(d)
        res["dominant"] = {"kernel": d["kernel"], "shape": d["shape"], "avg_us": d["avg_us"], "launches_per_step": d["launches"] / 3.0,
                           "bound": "mfma" if mf > hbm else "hbm", "frac": max(mf, hbm), "hbm_frac": hbm, "mfma_frac": mf,
                           "share_of_step": d["ms"] / 3.0 / (el / steps * 1e3)}
        if d["work_unit"] == "pairs":       # a search kernel: neither roofline binds, instruction issue does
            res["dominant"].update({"bound": "valu_issue", "frac": None, "pair_tests_per_s": d["gwork_s"] * 1e9})
        res["kernels"] = [_kernel_row(d, 3.0, el / steps * 1e3) for d in ks[:10]]
    del net, fp, opt, x
    gc.collect()
    torch.cuda.empty_cache()
    return res


F16_PEAK_TFLOPS = 2500.0            # dense fp16 matrix peak (MI355X_MICROARCH.md), the pipe knn_f16_kernel's filter runs on


def _kernel_row(d, steps, ms_per_step, traffic=None):
    """one row of a per-kernel table: time, share of the step, and the fraction of the roofline that binds the kernel --
    HBM or the matrix pipe it runs on for the streaming / MFMA kernels; for the search kernels (pair tests: instruction
    issue binds) the pair rate, the fp32-VALU fraction of a 9-lane-op pair test and, for the 64-channel
    kNN graph, its distance flops against the fp16 matrix pipe its filter runs on"""
    hbm, mf = d["gbs"] / HBM_PEAK_GBS, _mfma_frac(d)
    row = {"kernel": d["kernel"], "shape": d["shape"], "avg_us": d["avg_us"], "launches_per_step": d["launches"] / steps,
           "ms_per_step": d["ms"] / steps, "share_of_step": d["ms"] / steps / ms_per_step,
           "hbm_frac": hbm, "mfma_frac": mf, "bound": "mfma" if mf > hbm else "hbm", "bound_frac": max(hbm, mf),
           "pipe": ("bf16 x 6 (split operands)" if _split_operands(d) else
                    "f32 mfma (dW) + bf16 x 6 (dX)" if _half_split(d) else ("f32 mfma" if d["work_unit"] == "flop" else None))}
    if d["work_unit"] == "pairs":
        t = d["avg_us"] * 1e-6
        row.update({"bound": "valu_issue", "pair_tests_per_s": d["gwork_s"] * 1e9,
                    "bound_frac": d["work"] * QBP_VALU_OPS_PER_PAIR / t / VALU_LANE_OPS_PER_S})
        if d["kernel"].startswith("pcops_knn_graph") and len(d["shape"]) >= 3 and d["shape"][2] >= 64:
            row["f16_mfma_frac"] = 2.0 * d["work"] * d["shape"][2] / t / 1e12 / F16_PEAK_TFLOPS
    if traffic is not None:
        row["traffic"] = traffic
    return row


DUMP_MAX_BYTES = 64 << 20           # --dump-outputs: all arrays of one run together


def dump_outputs(dirname, arrays):
    """--dump-outputs DIR: every array as DIR/<name>.npy in float32.  The byte budget is split evenly over the arrays;
    an array larger than its share is written as a fixed sample of its flattened elements (the same seeded index set
    for the same size, so two builds' files compare element for element)."""
    os.makedirs(dirname, exist_ok=True)
    cap = DUMP_MAX_BYTES // 4 // len(arrays)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > cap:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), a)


def _shared_gpu_debug():
    """PCOPS_BENCH_SHARED_GPU=1: every rank on cuda:0 over gloo -- exercises the N > 1 control flow (barriers, gathers,
    the two measurement passes) on a one-GPU box.  The line is tagged `shared_gpu_debug`; its value means nothing."""
    return os.environ.get("PCOPS_BENCH_SHARED_GPU", "0") == "1"


def _self_launch(args):
    """`python bench.py --gpus N` with no rank environment: start the N ranks through torch.distributed.run."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not _shared_gpu_debug():
        raise SystemExit("bench.py: --gpus %d requested but only %d GPU(s) are visible" % (args.gpus, ndev))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="pointnet2_cls_ssg", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the config's)")
    ap.add_argument("--num_point", type=int, default=0)
    ap.add_argument("--kind", default="surface", choices=["surface", "ball"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--forward-only", action="store_true", help="eval-mode forward throughput (not the metric)")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the secondary measurements (eval forward, kind=ball, rotate+jitter in the step)")
    ap.add_argument("--augment", action="store_true",
                    help="put the device-side rotate + jitter of the input pipeline (provider.py) inside the timed step")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N > 1: ONE all-reduce of the flat gradient bucket after the backward pass instead of ranges "
                         "issued while it runs")
    ap.add_argument("--sync_bn", action="store_true", help="all-reduce the BN batch statistics over the ranks")
    ap.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible backward passes (pcops_set_deterministic); reported in config, not the metric run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy: "
                         "logits, loss, flat gradient and batch-norm moving statistics (--forward-only: logits); that "
                         "step starts from the seeded initial training state")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench.py needs the MI355X (the HIP path has no CPU fallback)"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(args)
    rank, world, local = D.init_from_env("gloo" if _shared_gpu_debug() else None)
    if _shared_gpu_debug():
        local = 0
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the process group has %d rank(s) (WORLD_SIZE=%s); refusing to "
                         "report a number for a different world size" % (args.gpus, world, os.environ.get("WORLD_SIZE")))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    _lib.load()
    torch.manual_seed(4321 + rank)              # the global generators (dropout masks): the same inputs in every run

    import gc
    import importlib
    from scanobjectnn_amd import provider
    modpath, has_mask, cfg_batch, cfg_n = MODELS[args.model]
    mod = importlib.import_module(modpath)
    B = args.batch or cfg_batch
    N = args.num_point or cfg_n
    D.SYNC_BN = bool(args.sync_bn) and world > 1
    if args.deterministic:
        from scanobjectnn_amd import _lib as _pl
        _pl.set_deterministic(True)

    def make_inputs(kind):
        xx = torch.from_numpy(synth_clouds(B, N, seed=1234 + rank, kind=kind)).to(dev)
        yy = torch.from_numpy(synth_labels(B, seed=1234 + rank)).to(dev)
        mm = torch.from_numpy(synth_masks(B, N, seed=1234 + rank)).to(dev) if has_mask else None
        return xx, yy, mm

    inputs = {"x": None}
    inputs["x"], y, mask = make_inputs(args.kind)

    net = Model(mod.get_model, device=dev, seed=0).build(inputs["x"][:2].contiguous())
    fp = TU.FlatParams(net)
    D.broadcast_(fp.flat)                       # identical replicas
    if not args.no_overlap:
        fp.enable_overlap(world)                # no-op for one rank
    opt = TU.TFAdam(fp)
    global_batch = B * world
    state = {"step": 0, "augment": bool(args.augment)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321 + rank)
    ar_events = []                              # (start, end) HIP events around the gradient all-reduce
    # --dump-outputs: the last timed step starts from the seeded initial training state, so that what it computes depends
    # on the arguments alone -- not on the summation order of the float atomics of the steps before it, which training
    # would carry forward and Adam amplify (a gradient that is exactly 0 but for rounding still moves its variable by ~lr)
    initial = [t.clone() for t in [fp.flat, opt.m, opt.v] + list(net.buffers())] if args.dump_outputs else None

    @torch.no_grad()
    def restore_initial_state():
        for dst, src in zip([fp.flat, opt.m, opt.v] + list(net.buffers()), initial):
            dst.copy_(src)
        opt.t = 0
        state["step"] = 0
        torch.manual_seed(4321 + rank)
        gen.manual_seed(4321 + rank)

    def train_step():
        s = state["step"]
        lr = TU.get_learning_rate(s, global_batch)
        bn_decay = TU.get_bn_decay(s, global_batch)
        x = inputs["x"]
        if state["augment"]:                    # §8f-1: the reference's per-batch rotate + jitter, on the device
            x = provider.jitter_point_cloud(provider.rotate_point_cloud(x, generator=gen), generator=gen).contiguous()
        fp.begin_step()
        out = net(x, is_training=True, bn_decay=bn_decay)
        if has_mask:
            loss = mod.get_loss(out[0], out[1], y, mask)[0]
        else:
            loss = mod.get_loss(out[0], y, out[1])
        if args.dump_outputs:
            state["out"] = (out[0].detach(), loss.detach())
        loss.backward()
        if world > 1:
            # the ranges of the flat bucket whose gradients the backward pass finished early are already travelling
            # (FlatParams.enable_overlap); the events bracket what is left EXPOSED: the last range + the waits
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fp.collect_mean(world)
            e1.record()
            ar_events.append((e0, e1))
        else:
            fp.collect()
        opt.step(lr)
        state["step"] = s + 1
        return loss

    def fwd_step():
        with torch.no_grad():
            out = net(inputs["x"], is_training=False)
        if args.dump_outputs:
            state["out"] = (out[0], None)
        return out

    def measure(step, steps, warmup, with_kernels, only=None, before_last=None):
        """W untimed steps, then exactly K steps between barrier + synchronize on both sides; max over ranks.
        before_last: called ahead of the last timed step"""
        for _ in range(warmup):
            step()
        # the host only has to stay ahead of the GPU: a generation-2 garbage collection in the middle of the timed
        # region (tens of ms with the autograd graphs of a step alive) would let the device queue run dry
        gc.collect()
        gc.disable()
        timer = KernelTimer(only) if with_kernels else None
        if timer:
            _lib._hooks.append(timer)
        del ar_events[:]
        D.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # host time per step is taken over the first few steps: once the launch queue is full (a few thousand launches:
        # 20+ steps of this model) every further launch waits for the GPU, and the average over all K steps drifts from
        # the host's own cost (3.6 ms) towards the GPU's step time
        nhost = min(steps, 10)
        host_elapsed = 0.0
        for i in range(steps):
            if before_last is not None and i + 1 == steps:
                before_last()
            step()
            if i + 1 == nhost:
                host_elapsed = (time.perf_counter() - t0) * steps / nhost     # scaled to K steps (reported per step)
        torch.cuda.synchronize()
        local_elapsed = time.perf_counter() - t0
        D.barrier()
        elapsed = time.perf_counter() - t0
        gc.enable()
        if timer:
            _lib._hooks.remove(timer)
        return D.max_over_ranks(elapsed, dev), local_elapsed, host_elapsed, (timer.summary() if timer else [])

    step = fwd_step if args.forward_only else train_step
    # pass 1 (not the metric): every libpcops launch bracketed by HIP events -> the per-kernel table, and which kernel
    # dominates.  pass 2 (the metric): W warm-up + exactly K timed steps in which only the DOMINANT kernel's launches
    # carry events -- its duration is measured live inside the timed region, the other ~160 launches run unbracketed.
    profile_steps = max(3, min(10, args.steps))
    _, _, _, kernels = measure(step, profile_steps, args.warmup, True)
    # the roofline object is about a kernel an HBM / MFMA roofline binds: the search kernels (pair tests: kNN graph, ball query,
    # FPS) are instruction-issue bound and are reported in `kernels` with their pair rate instead
    roofed = [d for d in kernels if d["work_unit"] != "pairs"]
    dom_key = (roofed[0]["kernel"], roofed[0]["shape"]) if roofed else None
    clock = None
    if rank == 0 and not os.environ.get("PCOPS_BENCH_NO_CLOCK"):
        with ClockPoller() as poller:
            elapsed, local_elapsed, host_elapsed, dom_live = measure(step, args.steps, args.warmup, dom_key is not None, dom_key,
                                                                     restore_initial_state if args.dump_outputs else None)
        clock = poller.summary()
    else:
        elapsed, local_elapsed, host_elapsed, dom_live = measure(step, args.steps, args.warmup, dom_key is not None, dom_key,
                                                                     restore_initial_state if args.dump_outputs else None)
    if args.dump_outputs and rank == 0:
        # before anything below steps the model again or swaps the input batch
        logits, loss = state["out"]
        arrays = {"logits": logits}
        if loss is not None:
            # not the parameters after the update: Adam maps rounding noise in an exactly-0 gradient to a step of ~lr
            arrays.update(loss=loss, grad=fp.grad, bn_moving_stats=torch.cat([b.reshape(-1) for b in net.buffers()]))
        dump_outputs(args.dump_outputs, arrays)
    # N > 1: the SAME invocation also measures rank 0 running alone (no collective, the other ranks parked at a barrier), so a
    # scaling curve built from the per-N lines has its own single-GPU baseline from the same box, build and clock state
    solo = None
    if world > 1 and not args.forward_only:
        D.barrier()
        if rank == 0:
            def solo_step():
                s_ = state["step"]
                fp.begin_step()
                fp._armed = False               # no gradient ranges leave: this is the one-GPU step
                out = net(inputs["x"], is_training=True, bn_decay=TU.get_bn_decay(s_, B))
                loss = mod.get_loss(out[0], out[1], y, mask)[0] if has_mask else mod.get_loss(out[0], y, out[1])
                loss.backward()
                fp.collect()
                opt.step(TU.get_learning_rate(s_, B))
                state["step"] = s_ + 1
            keep_sync = D.SYNC_BN
            D.SYNC_BN = False
            for _ in range(min(args.warmup, 3)):
                solo_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                solo_step()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            D.SYNC_BN = keep_sync
            solo = {"value": B * args.steps / el, "unit": "clouds/s", "ms_per_step": el / args.steps * 1e3, "n_gpus": 1,
                    "note": "rank 0 alone in this invocation (other ranks idle): the N = 1 point of the scaling curve"}
        D.barrier()
    ar_ms = [a.elapsed_time(b) for a, b in ar_events]
    per_rank = D.gather_floats(B * args.steps / local_elapsed, dev)      # every rank's own clouds/s
    ar_all = D.gather_floats(sum(ar_ms) / max(len(ar_ms), 1), dev)
    rccl_ranks = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1

    # ---- secondary measurements (single GPU only; never part of `value`)
    extras = {}
    if world == 1 and not args.no_extras and not args.forward_only:
        k2 = max(5, min(20, args.steps))
        e, _, _, _ = measure(fwd_step, k2, 3, False)
        extras["forward_eval_clouds_per_s"] = B * k2 / e
        other = "ball" if args.kind == "surface" else "surface"
        keep = inputs["x"]
        inputs["x"] = make_inputs(other)[0]
        e, _, _, _ = measure(train_step, k2, 3, False)
        extras["train_clouds_per_s_kind_%s" % other] = B * k2 / e
        e, _, _, _ = measure(fwd_step, k2, 3, False)
        extras["forward_eval_clouds_per_s_kind_%s" % other] = B * k2 / e
        inputs["x"] = keep
        if not state["augment"]:
            state["augment"] = True
            e, _, _, _ = measure(train_step, k2, 3, False)
            extras["train_clouds_per_s_with_rotate_jitter"] = B * k2 / e
            state["augment"] = False
        extras["steps_each"] = k2
        if args.model == "pointnet2_cls_ssg" and not args.batch and not args.num_point and not args.deterministic:
            # BASELINE.json configs[2..4] at their per-GPU batch, on the same library (not the metric)
            extras["models"] = {}
            for other_model in ("dgcnn", "pointnet2_cls_bga", "pointnet2_cls_msg"):
                try:
                    extras["models"][other_model] = side_model(other_model, dev)
                except Exception as ex:       # a reported extra: never lose the bench line over it
                    extras["models"][other_model] = {"error": repr(ex)}

    # ---- ball query: the pair tests the kernel actually executes (it stops a query at its nsample-th hit) and the
    # fp32-VALU bound next to the HBM figure (brute force is VALU bound, both are reported)
    qbp = None
    if rank == 0 and args.model.startswith("pointnet2_cls_ssg"):
        qbp = _ball_query_fractions(inputs["x"], kernels)

    if rank != 0:
        return
    value = global_batch * args.steps / elapsed
    for d in kernels:
        d["hbm_frac"] = d["gbs"] / HBM_PEAK_GBS
        d["mfma_frac"] = _mfma_frac(d)
        d["pipe"] = ("bf16 x 6 (split operands)" if _split_operands(d) else
                     "f32 mfma (dW) + bf16 x 6 (dX)" if _half_split(d) else ("f32 mfma" if d["work_unit"] == "flop" else None))
        d["pipe_busy_frac"] = _pipe_busy(d)
        d["bound_frac"] = max(d["hbm_frac"], d["mfma_frac"])
    for d in dom_live:
        d["hbm_frac"] = d["gbs"] / HBM_PEAK_GBS
        d["mfma_frac"] = _mfma_frac(d)
    dom = dom_live[0] if dom_live else (roofed[0] if roofed else None)       # measured inside the timed region
    roofline = None
    if dom is not None:
        # the binding roofline of the dominant kernel = the one it sits closer to: HBM for the streaming
        # kernels; for the MFMA GEMMs whichever of (algorithmic bytes / 8 TB/s, flops / 157.3 TF/s) is larger
        hbm_frac, mfma_frac = dom["hbm_frac"], dom["mfma_frac"]
        traffic = _measured_traffic(dom)     # PMC bytes of this kernel from the committed profile of the same command (below)
        split = _split_operands(dom)
        if mfma_frac > hbm_frac and split:       # six bf16 products per algorithmic fp32 product, on the bf16 pipe
            roofline = {"bound": "mfma", "achieved": 6.0 * dom["gwork_s"] / 1e3, "peak": BF16_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": mfma_frac, "traffic": traffic, "pipe": "bf16 x 6 (split operands)"}
        elif mfma_frac > hbm_frac:
            roofline = {"bound": "mfma", "achieved": dom["gwork_s"] / 1e3, "peak": F32_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": mfma_frac, "traffic": traffic}
        else:
            roofline = {"bound": "hbm", "achieved": dom["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": hbm_frac, "traffic": traffic}
        roofline.update({"kernel": dom["kernel"], "shape": dom["shape"], "avg_launch_us": dom["avg_us"],
                         "launches": dom["launches"], "algorithmic_bytes_per_launch": dom["bytes"],
                         "algorithmic_flops_per_launch": dom["work"] if dom["work_unit"] == "flop" else None,
                         "hbm_frac": hbm_frac, "mfma_frac": mfma_frac,
                         # `traffic` is NOT measured by this process (PMC counters need their own rocprofv3 passes): it is this
                         # kernel's FETCH x 2 + WRITE bytes from the committed passes of the same command, named here
                         "traffic_source": ("%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py` (tools/collect_traffic.py), "
                                            "not collected in this run" % _measured_traffic.source) if traffic is not None else None,
                         # which pipe(s) the launch's products run on, and the share of the launch the matrix pipe is busy
                         # at its nominal rate (`frac` prices the ALGORITHMIC fp32 flops against the fp32-input peak)
                         "pipe": ("f32 mfma (dW) + bf16 x 6 (dX)" if _half_split(dom) else
                                  "bf16 x 6 (split operands)" if split else "f32 mfma"),
                         "pipe_busy_frac": _pipe_busy(dom),
                         # `frac` is priced at the boost clock; the same launch against the peak at the clock the chip
                         # actually held over the timed region (matrix-bound kernels only: HBM does not follow sclk)
                         "frac_at_measured_clock": (roofline["frac"] * BOOST_MHZ / clock["sclk_mhz"]
                                                    if clock and roofline["bound"] == "mfma" else None),
                         "share_of_step": dom["ms"] / (elapsed * 1e3),
                         # ceilings measured on this chip (tools/ubench, MI355X_MICROARCH.md): what `peak` is in practice
                         "peak_measured": {"mfma_f32_tflops": MEASURED_F32_MFMA_TFLOPS, "hbm_gbs": MEASURED_HBM_GBS},
                         "frac_of_measured_peak": (mfma_frac if (mfma_frac > hbm_frac and split) else
                                                   dom["gwork_s"] / 1e3 / MEASURED_F32_MFMA_TFLOPS
                                                   if mfma_frac > hbm_frac else dom["gbs"] / MEASURED_HBM_GBS)})
    if roofline is not None:
        # the object above names ONE kernel by a fixed rule -- the largest time per step in pass 1 among the kernels an HBM /
        # MFMA roofline binds; two kernels within a few per cent of each other may swap places from box to box (r04: the
        # one-pass backward at 0.67, r05: the 256 -> 128 data gradient at 0.47 -- same tree), so the three largest are listed
        roofline["rule"] = "largest time per step (pass 1) among the kernels a roofline binds; top3 lists the first three"
        roofline["top3"] = [_kernel_row(d, float(profile_steps), elapsed / args.steps * 1e3, _measured_traffic(d))
                            for d in roofed[:3]]
    line = {
        "metric": "point-clouds/sec fwd+bwd at B×2048×3, 15-cls" if not args.forward_only
                  else "point-clouds/sec forward (eval) at B×2048×3, 15-cls",
        "value": value, "unit": "clouds/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "host_enqueue_ms_per_step": host_elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s PB_T50_RS-shaped synthetic clouds (%s), %d pts, batch %d per GPU, "
                               "train step = %sfwd+bwd+allreduce+Adam"
                               % (args.model, args.kind, N, B, "rotate+jitter+" if args.augment else ""),
                   "global_batch": global_batch, "num_point": N, "parallelism": "dp%d" % world,
                   "sync_bn": bool(D.SYNC_BN), "deterministic": bool(args.deterministic),
                   **({"shared_gpu_debug": True} if _shared_gpu_debug() else {})},
        "rccl_ranks": rccl_ranks,
        "per_rank_clouds_per_s": per_rank,
        "allreduce_overlapped": bool(world > 1 and not args.no_overlap),   # ms below = the EXPOSED part (last range + waits)
        "allreduce_ms_per_step": max(ar_all) if world > 1 else 0.0,
        "allreduce_share_of_step": (max(ar_all) / (elapsed / args.steps * 1e3)) if world > 1 else 0.0,
        "roofline": roofline,
        "clock": clock,
        "kernels_steps": profile_steps,
        "kernels_pass": "separate untimed pass of %d steps with every launch bracketed by HIP events; the timed region "
                        "brackets the dominant kernel only (roofline)" % profile_steps,
        "kernels": [{k: d[k] for k in ("kernel", "shape", "launches", "avg_us", "gbs", "gwork_s", "work_unit",
                                        "hbm_frac", "mfma_frac", "bound_frac", "pipe", "pipe_busy_frac")} for d in kernels[:24]],
    }
    if solo:
        line["single_gpu_same_invocation"] = solo
    if extras:
        line["extras"] = extras
    if qbp:
        line["ball_query"] = qbp
    if not args.no_cpu_baseline and world == 1:
        line["cpu_baseline"] = cpu_baseline(args.model, N)
        # SURVEY.md section 8(d) asks for the op-level reference-CPU figures in THIS record: a failure here is a failure
        # of the bench run (non-zero exit), not an {"error": ...} entry nobody reads (round 3's driver line lost them to
        # a ctypes race, fixed in oracle/oracle.py and pinned by tests/test_oracle_threads_cpu.py)
        line["cpu_baseline"]["ops"] = cpu_ops_baseline()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
