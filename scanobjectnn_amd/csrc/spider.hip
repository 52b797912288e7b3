// spider.hip -- the SpiderConv layer of SpiderCNN (reference SpiderCNN/utils/tf_util.py:127-236, :407-429) on gfx950.
//
// One layer, P = b n centre points, k neighbours (self first), T = 5 Taylor channels:
//   g[p,j,t]  = sum_m theta[m,t] phi_m(delta[p,j]) + tbias[t]                  (pcops_spider_taylor_fwd)
//   y[p,o]    = bias[o] + sum_{j,c,t} F[idx[p,j],c] g[p,j,t] W[(j C + c) T + t, o] (pcops_spider_conv_fwd)
//   out       = relu(group_norm(y))                                              (pcops_group_norm_relu_fwd)
// The expanded operand A[p,(j,c,t)] = F[idx[p,j],c] g[p,j,t] (the reference's expand_dims / tile / reshape, :219-223)
// is never written to memory: the product kernels form its tile in LDS from the gathered rows of F and the g rows.
//
// Tiles: 16 channels x 5 Taylor channels = 80 K entries per block, i.e. one (j, 16-channel) slice; channels past C are
// zero on both operands.  fp32 MFMA (v_mfma_f32_16x16x4_f32): A[l&15][k=l>>4], B[k=l>>4][l&15],
// C/D col = l&15, row = 4 (l>>4) + reg.  Every sum is taken in a fixed order: no float atomics anywhere in this file.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kT = 5;          // Taylor channels (the reference's taylor_channel)
constexpr int kMono = 19;      // monomials of the cubic Taylor kernel
constexpr int kCB = 16;        // channels per K block
constexpr int kKB = kCB * kT;  // 80 K entries per block
constexpr int kBM = 64;        // rows (points) per tile
constexpr int kBN = 64;        // output columns per tile
constexpr int kThreads = 256;
constexpr int kTaylorBlocks = 256;   // partial rows of the dtheta reduction


// phi_m(d), m in the order x y z xyz | xy yz xz | xx yy zz | xxy xyy xxz | xzz yyz yzz | xxx yyy zzz
__device__ __forceinline__ void monomials(float X, float Y, float Z, float *ph) {
    const float xx = X * X, yy = Y * Y, zz = Z * Z, xy = X * Y, yz = Y * Z, xz = X * Z;
    ph[0] = X; ph[1] = Y; ph[2] = Z; ph[3] = xy * Z;
    ph[4] = xy; ph[5] = yz; ph[6] = xz;
    ph[7] = xx; ph[8] = yy; ph[9] = zz;
    ph[10] = xx * Y; ph[11] = xy * Y; ph[12] = xx * Z;
    ph[13] = xz * Z; ph[14] = yy * Z; ph[15] = yz * Z;
    ph[16] = xx * X; ph[17] = yy * Y; ph[18] = zz * Z;
}

__global__ void __launch_bounds__(kThreads) taylor_fwd_kernel(long long rows, const float *__restrict__ delta,
                                                              const float *__restrict__ theta,
                                                              const float *__restrict__ tbias, float *__restrict__ g) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows) return;
    float ph[kMono];
    monomials(delta[3 * r], delta[3 * r + 1], delta[3 * r + 2], ph);
#pragma unroll
    for (int t = 0; t < kT; ++t) {
        float s = tbias[t];
#pragma unroll
        for (int m = 0; m < kMono; ++m) s = fmaf(theta[m * kT + t], ph[m], s);
        g[r * kT + t] = s;
    }
}

// partial[blk][m * T + t] (m = 19: the bias) = sum over this block's rows, rows taken in a fixed stride pattern
__global__ void __launch_bounds__(kThreads) taylor_bwd_partial_kernel(long long rows, const float *__restrict__ delta,
                                                                      const float *__restrict__ dg,
                                                                      float *__restrict__ partial) {
    constexpr int Q = (kMono + 1) * kT;   // 100
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < rows; r += stride) {
        float ph[kMono + 1];
        monomials(delta[3 * r], delta[3 * r + 1], delta[3 * r + 2], ph);
        ph[kMono] = 1.f;
        float d[kT];
#pragma unroll
        for (int t = 0; t < kT; ++t) d[t] = dg[r * kT + t];
#pragma unroll
        for (int m = 0; m <= kMono; ++m)
#pragma unroll
            for (int t = 0; t < kT; ++t) acc[m * kT + t] = fmaf(ph[m], d[t], acc[m * kT + t]);
    }
    constexpr int QC = 25;                 // quantities per LDS round
    __shared__ float red[QC][kThreads + 1];
#pragma unroll
    for (int q0 = 0; q0 < Q; q0 += QC) {
#pragma unroll
        for (int q = 0; q < QC; ++q) red[q][threadIdx.x] = acc[q0 + q];
        __syncthreads();
        if (threadIdx.x < QC) {
            float s = 0.f;
            for (int i = 0; i < kThreads; ++i) s += red[threadIdx.x][i];
            partial[(size_t)blockIdx.x * Q + q0 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

__global__ void taylor_bwd_final_kernel(int nblk, const float *__restrict__ partial, float *__restrict__ dtheta,
                                        float *__restrict__ dtbias) {
    constexpr int Q = (kMono + 1) * kT;
    const int q = threadIdx.x;
    if (q >= Q) return;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += partial[(size_t)i * Q + q];
    if (q < kMono * kT) dtheta[q] = s;
    else dtbias[q - kMono * kT] = s;
}

// ---------------------------------------------------------------------------------------------- forward contraction
// grid (ceil(n / 64), ceil(o / 64), b); 4 waves, each a 32 x 32 quarter of the 64 x 64 output tile
__global__ void __launch_bounds__(kThreads) conv_fwd_kernel(int n, int C, int k, int O, const float *__restrict__ F,
                                                            const int *__restrict__ idx, const float *__restrict__ g,
                                                            const float *__restrict__ W,
                                                            const float *__restrict__ bias, float *__restrict__ y) {
    __shared__ float As[kKB][kBM + 4];   // As[kk][row]
    __shared__ float Bs[kKB][kBN + 4];   // Bs[kk][col]
    __shared__ int sIdx[kBM];
    __shared__ float sG[kBM][kT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * kBM, col0 = blockIdx.y * kBN, cloud = blockIdx.z;
    const size_t cbase = (size_t)cloud * n;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j = 0; j < k; ++j) {
        __syncthreads();
        if (tid < kBM) {
            const int p = row0 + tid;
            sIdx[tid] = p < n ? idx[(cbase + p) * k + j] : 0;
        }
        for (int e = tid; e < kBM * kT; e += kThreads) {
            const int r = e / kT, t = e - r * kT, p = row0 + r;
            sG[r][t] = p < n ? g[((cbase + p) * k + j) * kT + t] : 0.f;
        }
        __syncthreads();
        for (int c0 = 0; c0 < C; c0 += kCB) {
            for (int e = tid; e < kBM * kCB; e += kThreads) {
                const int r = e >> 4, cc = e & 15, c = c0 + cc;
                const float v = (row0 + r < n && c < C) ? F[(cbase + sIdx[r]) * C + c] : 0.f;
#pragma unroll
                for (int t = 0; t < kT; ++t) As[cc * kT + t][r] = v * sG[r][t];
            }
            const size_t wrow0 = ((size_t)j * C + c0) * kT;
            for (int e = tid; e < kKB * kBN; e += kThreads) {
                const int kk = e >> 6, cl = e & 63;
                const bool ok = c0 + kk / kT < C && col0 + cl < O;
                Bs[kk][cl] = ok ? W[(wrow0 + kk) * O + col0 + cl] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int ks = 0; ks < kKB / 4; ++ks) {
                const int kk = ks * 4 + (lane >> 4);
                float a[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = As[kk][wr + i * 16 + (lane & 15)];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) bv[jj] = Bs[kk][wc + jj * 16 + (lane & 15)];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[jj], acc[i][jj], 0, 0, 0);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int col = col0 + wc + jj * 16 + (lane & 15);
            if (col >= O) continue;
            const float bb = bias ? bias[col] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = row0 + wr + i * 16 + (lane >> 4) * 4 + q;
                if (row < n) y[(cbase + row) * O + col] = acc[i][jj][q] + bb;
            }
        }
}

// ---------------------------------------------------------------------------------------------- weight gradient
// dW[(j C + c) T + t, o] = sum_p A[p,(j,c,t)] dY[p,o]; grid (k * ceil(C / 16), ceil(o / 64), splits).  Split s takes the
// rows [s chunk, (s + 1) chunk) of all b n rows in ascending 64-row steps; with splits > 1 it writes
// ws[s][K][O] (+ ws_db[s][O]) and wgrad_reduce_kernel adds the splits in ascending order.  The workgroups of K block 0
// also take the column sums of dY (db).  Each wave: 16 output columns x all 80 K rows (5 accumulators).
__global__ void __launch_bounds__(kThreads) conv_wgrad_kernel(int P, int n, int C, int k, int O, int chunk,
                                                              const float *__restrict__ F, const int *__restrict__ idx,
                                                              const float *__restrict__ g,
                                                              const float *__restrict__ dy, float *__restrict__ dw,
                                                              float *__restrict__ db) {
    __shared__ float At[kBM][kKB + 4];   // At[p][kk]
    __shared__ float Ds[kBM][kBN + 4];   // Ds[p][col]
    __shared__ int sIdx[kBM];
    __shared__ float sG[kBM][kT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cblocks = (C + kCB - 1) / kCB;
    const int j = blockIdx.x / cblocks, c0 = (blockIdx.x - j * cblocks) * kCB;
    const int col0 = blockIdx.y * kBN, split = blockIdx.z;
    const int pbeg = split * chunk, pend = min(P, pbeg + chunk);
    const bool do_db = db != nullptr && blockIdx.x == 0;
    f32x4 acc[5];
#pragma unroll
    for (int mi = 0; mi < 5; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;

    for (int p0 = pbeg; p0 < pend; p0 += kBM) {
        __syncthreads();
        if (tid < kBM) {
            const int p = p0 + tid;
            int v = 0;
            if (p < pend) v = (p / n) * n + idx[(size_t)p * k + j];   // global row of the neighbour
            sIdx[tid] = v;
        }
        for (int e = tid; e < kBM * kT; e += kThreads) {
            const int r = e / kT, t = e - r * kT, p = p0 + r;
            sG[r][t] = p < pend ? g[((size_t)p * k + j) * kT + t] : 0.f;
        }
        for (int e = tid; e < kBM * kBN; e += kThreads) {
            const int r = e >> 6, cl = e & 63, p = p0 + r;
            Ds[r][cl] = (p < pend && col0 + cl < O) ? dy[(size_t)p * O + col0 + cl] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < kBM * kCB; e += kThreads) {
            const int r = e >> 4, cc = e & 15, c = c0 + cc;
            const float v = (p0 + r < pend && c < C) ? F[(size_t)sIdx[r] * C + c] : 0.f;
#pragma unroll
            for (int t = 0; t < kT; ++t) At[r][cc * kT + t] = v * sG[r][t];
        }
        if (do_db && tid < kBN) {
            for (int r = 0; r < kBM; ++r) dbs += Ds[r][tid];
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < kBM / 4; ++ks) {
            const int pr = ks * 4 + (lane >> 4);
            const float bv = Ds[pr][wave * 16 + (lane & 15)];
#pragma unroll
            for (int mi = 0; mi < 5; ++mi)
                acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(At[pr][mi * 16 + (lane & 15)], bv, acc[mi], 0, 0, 0);
        }
    }
    const size_t K = (size_t)k * C * kT;
    float *out = gridDim.z > 1 ? dw + (size_t)split * K * O : dw;
    const int col = col0 + wave * 16 + (lane & 15);
    if (col < O) {
#pragma unroll
        for (int mi = 0; mi < 5; ++mi)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kk = mi * 16 + (lane >> 4) * 4 + q;
                if (c0 + kk / kT < C) out[(((size_t)j * C + c0) * kT + kk) * O + col] = acc[mi][q];
            }
    }
    if (do_db && tid < kBN && col0 + tid < O) db[(size_t)(gridDim.z > 1 ? split : 0) * O + col0 + tid] = dbs;
}

__global__ void wgrad_reduce_kernel(long long len, int splits, const float *__restrict__ ws, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= len) return;
    float s = 0.f;
    for (int q = 0; q < splits; ++q) s += ws[(size_t)q * len + i];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------- data gradient
// dA[p,(j,c,t)] = sum_o dY[p,o] W[(j C + c) T + t, o] for one (64-row tile, j), 16 channels at a time, reduced at once to
//   dfg[p,j,c] = sum_t dA g[p,j,t]   and   dg[p,j,t] = sum_c dA F[idx[p,j],c]   (c ascending).
// grid (ceil(n / 64), k, b); each wave: 16 rows x all 80 K entries (5 accumulators); dY / W streamed in 64-column steps.
__global__ void __launch_bounds__(kThreads) conv_dgrad_kernel(int n, int C, int k, int O, const float *__restrict__ F,
                                                              const int *__restrict__ idx, const float *__restrict__ g,
                                                              const float *__restrict__ W,
                                                              const float *__restrict__ dy, float *__restrict__ dfg,
                                                              float *__restrict__ dg) {
    __shared__ float Ds[kBM][kBN + 4];   // Ds[row][o]
    __shared__ float Ws[kBN][kKB + 4];   // Ws[o][kk]
    __shared__ float dAs[kBM][kKB + 1];
    __shared__ float Fs[kBM][kCB + 1];
    __shared__ int sIdx[kBM];
    __shared__ float sG[kBM][kT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * kBM, j = blockIdx.y, cloud = blockIdx.z;
    const size_t cbase = (size_t)cloud * n;
    if (tid < kBM) {
        const int p = row0 + tid;
        sIdx[tid] = p < n ? idx[(cbase + p) * k + j] : 0;
    }
    for (int e = tid; e < kBM * kT; e += kThreads) {
        const int r = e / kT, t = e - r * kT, p = row0 + r;
        sG[r][t] = p < n ? g[((cbase + p) * k + j) * kT + t] : 0.f;
    }
    float dgacc[2] = {0.f, 0.f};     // entries e = tid, tid + 256 of the (64 x 5) dg tile
    for (int c0 = 0; c0 < C; c0 += kCB) {
        f32x4 acc[5];
#pragma unroll
        for (int mi = 0; mi < 5; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
        const size_t wrow0 = ((size_t)j * C + c0) * kT;
        for (int o0 = 0; o0 < O; o0 += kBN) {
            __syncthreads();
            for (int e = tid; e < kBM * kBN; e += kThreads) {
                const int r = e >> 6, cl = e & 63;
                Ds[r][cl] = (row0 + r < n && o0 + cl < O) ? dy[(cbase + row0 + r) * O + o0 + cl] : 0.f;
            }
            for (int e = tid; e < kKB * kBN; e += kThreads) {
                const int kk = e >> 6, cl = e & 63;
                const bool ok = c0 + kk / kT < C && o0 + cl < O;
                Ws[cl][kk] = ok ? W[(wrow0 + kk) * O + o0 + cl] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int ks = 0; ks < kBN / 4; ++ks) {
                const int ol = ks * 4 + (lane >> 4);
                const float a = Ds[wave * 16 + (lane & 15)][ol];
#pragma unroll
                for (int mi = 0; mi < 5; ++mi)
                    acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ws[ol][mi * 16 + (lane & 15)], acc[mi], 0, 0, 0);
            }
        }
        // dA tile -> LDS (row = wave * 16 + 4 (lane >> 4) + q, kk = 16 mi + (lane & 15)), gathered F slice -> LDS
#pragma unroll
        for (int mi = 0; mi < 5; ++mi)
#pragma unroll
            for (int q = 0; q < 4; ++q) dAs[wave * 16 + (lane >> 4) * 4 + q][mi * 16 + (lane & 15)] = acc[mi][q];
        for (int e = tid; e < kBM * kCB; e += kThreads) {
            const int r = e >> 4, cc = e & 15, c = c0 + cc;
            Fs[r][cc] = (row0 + r < n && c < C) ? F[(cbase + sIdx[r]) * C + c] : 0.f;
        }
        __syncthreads();
        if (dfg) {
            for (int e = tid; e < kBM * kCB; e += kThreads) {
                const int r = e >> 4, cc = e & 15, c = c0 + cc, p = row0 + r;
                if (p >= n || c >= C) continue;
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < kT; ++t) s = fmaf(dAs[r][cc * kT + t], sG[r][t], s);
                dfg[((cbase + p) * k + j) * C + c] = s;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = tid + h * kThreads;
            if (e < kBM * kT) {
                const int r = e / kT, t = e - r * kT;
                const int ce = min(kCB, C - c0);
                float s = dgacc[h];
                for (int cc = 0; cc < ce; ++cc) s = fmaf(dAs[r][cc * kT + t], Fs[r][cc], s);
                dgacc[h] = s;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int e = tid + h * kThreads;
        if (e < kBM * kT) {
            const int r = e / kT, t = e - r * kT, p = row0 + r;
            if (p < n) dg[((cbase + p) * k + j) * kT + t] = dgacc[h];
        }
    }
}

// ---------------------------------------------------------------------------------------------- group norm + ReLU
// grid (groups, b): one workgroup per (cloud, group) of cg = C / groups contiguous channels over the cloud's n points.
// Two-pass moments (mean, then the mean of squared deviations), tree sums in a fixed order.
__device__ __forceinline__ float block_sum(float v, float *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kThreads) gn_fwd_kernel(int n, int C, int groups, float eps, const float *__restrict__ x,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float *__restrict__ y,
                                                          float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    __shared__ float red[kThreads];
    const int gi = blockIdx.x, cloud = blockIdx.y, cg = C / groups;
    const long long cnt = (long long)n * cg;
    const float *xb = x + (size_t)cloud * n * C + (size_t)gi * cg;
    float s = 0.f;
    for (long long e = threadIdx.x; e < cnt; e += kThreads) s += xb[(e / cg) * C + e % cg];
    const float mean = block_sum(s, red) / (float)cnt;
    float v = 0.f;
    for (long long e = threadIdx.x; e < cnt; e += kThreads) {
        const float d = xb[(e / cg) * C + e % cg] - mean;
        v = fmaf(d, d, v);
    }
    const float var = block_sum(v, red) / (float)cnt;
    const float rstd = 1.f / sqrtf(var + eps);
    float *yb = y + (size_t)cloud * n * C + (size_t)gi * cg;
    for (long long e = threadIdx.x; e < cnt; e += kThreads) {
        const int cc = (int)(e % cg), ch = gi * cg + cc;
        const size_t off = (e / cg) * C + cc;
        const float o = fmaf(gamma[ch], (xb[off] - mean) * rstd, beta[ch]);
        yb[off] = o > 0.f ? o : 0.f;
    }
    if (threadIdx.x == 0) {
        mean_out[(size_t)cloud * groups + gi] = mean;
        rstd_out[(size_t)cloud * groups + gi] = rstd;
    }
}

// gy = dout (y > 0); xhat = (x - mean) rstd; dx = rstd (gamma gy - mean(gamma gy) - xhat mean(gamma gy xhat));
// per-cloud channel sums sum_p gy xhat, sum_p gy -> ws[cloud][2][C] (summed over clouds by gn_bwd_final_kernel).
// The first nact = (256 / cg) cg threads walk the group's elements with stride nact, so each of them always sees
// channel tid % cg (cg <= 256); the rest idle in the sums.
__global__ void __launch_bounds__(kThreads) gn_bwd_kernel(int n, int C, int groups, const float *__restrict__ dout,
                                                          const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ mean_in,
                                                          const float *__restrict__ rstd_in, float *__restrict__ dx,
                                                          float *__restrict__ ws) {
    __shared__ float red[kThreads];
    __shared__ float red2[kThreads];
    const int gi = blockIdx.x, cloud = blockIdx.y, cg = C / groups;
    const int nact = (kThreads / cg) * cg;
    const long long cnt = (long long)n * cg;
    const size_t base = (size_t)cloud * n * C + (size_t)gi * cg;
    const float mean = mean_in[(size_t)cloud * groups + gi], rstd = rstd_in[(size_t)cloud * groups + gi];
    const int cc = threadIdx.x % cg, ch = gi * cg + cc;
    const float gm = gamma[ch];
    float sg = 0.f, sgx = 0.f;            // this thread's channel: sum gy, sum gy xhat
    if ((int)threadIdx.x < nact) {
        for (long long e = threadIdx.x; e < cnt; e += nact) {
            const size_t off = base + (e / cg) * C + cc;
            const float gy = y[off] > 0.f ? dout[off] : 0.f;
            sg += gy;
            sgx = fmaf(gy, (x[off] - mean) * rstd, sgx);
        }
    }
    red[threadIdx.x] = sg;
    red2[threadIdx.x] = sgx;
    __syncthreads();
    float csg = 0.f, csgx = 0.f;          // channel totals (thread cc < cg), ascending thread order
    if ((int)threadIdx.x < cg) {
        for (int i = threadIdx.x; i < nact; i += cg) {
            csg += red[i];
            csgx += red2[i];
        }
        ws[((size_t)cloud * 2 + 0) * C + ch] = csgx;
        ws[((size_t)cloud * 2 + 1) * C + ch] = csg;
    }
    __syncthreads();
    const float s1 = block_sum((int)threadIdx.x < cg ? gm * csg : 0.f, red);
    const float s2 = block_sum((int)threadIdx.x < cg ? gm * csgx : 0.f, red);
    const float m1 = s1 / (float)cnt, m2 = s2 / (float)cnt;
    for (long long e = threadIdx.x; e < cnt; e += kThreads) {
        const int ec = (int)(e % cg);
        const size_t off = base + (e / cg) * C + ec;
        const float gy = y[off] > 0.f ? dout[off] : 0.f;
        const float xh = (x[off] - mean) * rstd;
        dx[off] = rstd * (fmaf(gamma[gi * cg + ec], gy, -m1) - xh * m2);
    }
}

__global__ void gn_bwd_final_kernel(int b, int C, const float *__restrict__ ws, float *__restrict__ dgamma,
                                    float *__restrict__ dbeta) {
    const int ch = blockIdx.x * kThreads + threadIdx.x;
    if (ch >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int i = 0; i < b; ++i) {
        sg += ws[((size_t)i * 2 + 0) * C + ch];
        sb += ws[((size_t)i * 2 + 1) * C + ch];
    }
    dgamma[ch] = sg;
    dbeta[ch] = sb;
}

int taylor_blocks(long long rows) { return (int)std::min<long long>(kTaylorBlocks, std::max(1u, cdiv(rows, kThreads))); }

// split count of the weight gradient: enough workgroups to fill the device, at most 16, at least 64 rows per split
int wgrad_splits(int b, int n, int c, int k, int o) {
    const long long P = (long long)b * n;
    const long long nwg = (long long)k * ((c + kCB - 1) / kCB) * ((o + kBN - 1) / kBN);
    long long s = (1024 + nwg - 1) / nwg;
    s = std::min<long long>(s, 16);
    s = std::min<long long>(s, (P + kBM - 1) / kBM);
    return (int)std::max<long long>(s, 1);
}

int check_conv(int b, int n, int c, int k, int t, int o) {
    PCOPS_REQUIRE_SHAPE(b >= 0 && n > 0 && c > 0 && o > 0);
    PCOPS_REQUIRE_ARG(k > 0 && k <= n && t > 0);
    if (k > 64 || t != kT || c > 256 || o % 16 != 0 || o > 512) return PCOPS_ERR_UNSUPPORTED;
    if ((long long)b * n * k * (c > kT ? c : kT) >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}

}  // namespace

extern "C" int pcops_spider_taylor_fwd(long long rows, int t, const float *delta, const float *theta,
                                       const float *tbias, float *g, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(rows >= 0);
    if (t != kT) return PCOPS_ERR_UNSUPPORTED;
    if (rows == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(delta); PCOPS_REQUIRE_PTR(theta); PCOPS_REQUIRE_PTR(tbias); PCOPS_REQUIRE_PTR(g);
    hipLaunchKernelGGL(taylor_fwd_kernel, dim3(cdiv(rows, kThreads)), dim3(kThreads), 0, as_stream(stream), rows, delta,
                       theta, tbias, g);
    return pcops_launch_status();
}

extern "C" unsigned long long pcops_spider_taylor_bwd_workspace_bytes(long long rows, int t) {
    if (rows <= 0 || t != kT) return 0;
    return (unsigned long long)taylor_blocks(rows) * (kMono + 1) * kT * sizeof(float);
}

extern "C" int pcops_spider_taylor_bwd(long long rows, int t, const float *delta, const float *dg, float *dtheta,
                                       float *dtbias, void *workspace, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(rows >= 0);
    if (t != kT) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(dtheta); PCOPS_REQUIRE_PTR(dtbias);
    hipStream_t s = as_stream(stream);
    if (rows == 0) {
        (void)pcops_zero_async(dtheta, kMono * kT * sizeof(float), s);
        (void)pcops_zero_async(dtbias, kT * sizeof(float), s);
        return pcops_launch_status();
    }
    PCOPS_REQUIRE_PTR(delta); PCOPS_REQUIRE_PTR(dg); PCOPS_REQUIRE_PTR(workspace);
    const int nblk = taylor_blocks(rows);
    float *partial = static_cast<float *>(workspace);
    hipLaunchKernelGGL(taylor_bwd_partial_kernel, dim3(nblk), dim3(kThreads), 0, s, rows, delta, dg, partial);
    hipLaunchKernelGGL(taylor_bwd_final_kernel, dim3(1), dim3(128), 0, s, nblk, partial, dtheta, dtbias);
    return pcops_launch_status();
}

extern "C" int pcops_spider_conv_fwd(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx,
                                     const float *g, const float *w, const float *bias, float *y,
                                     pcops_stream_t stream) {
    const int st = check_conv(b, n, c, k, t, o);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(feat); PCOPS_REQUIRE_PTR(idx); PCOPS_REQUIRE_PTR(g); PCOPS_REQUIRE_PTR(w); PCOPS_REQUIRE_PTR(y);
    hipLaunchKernelGGL(conv_fwd_kernel, dim3(cdiv(n, kBM), cdiv(o, kBN), b), dim3(kThreads), 0, as_stream(stream), n, c,
                       k, o, feat, idx, g, w, bias, y);
    pcops_note_pipe(0);
    return pcops_launch_status();
}

extern "C" unsigned long long pcops_spider_conv_wgrad_workspace_bytes(int b, int n, int c, int k, int t, int o) {
    if (check_conv(b, n, c, k, t, o) != PCOPS_OK || b == 0) return 0;
    const int s = wgrad_splits(b, n, c, k, o);
    if (s <= 1) return 0;
    return (unsigned long long)s * ((unsigned long long)k * c * kT * o + o) * sizeof(float);
}

extern "C" int pcops_spider_conv_wgrad(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx,
                                       const float *g, const float *dy, float *dw, float *dbias, void *workspace,
                                       pcops_stream_t stream) {
    const int st = check_conv(b, n, c, k, t, o);
    if (st != PCOPS_OK) return st;
    PCOPS_REQUIRE_PTR(dw);
    hipStream_t s = as_stream(stream);
    const size_t K = (size_t)k * c * kT;
    if (b == 0) {
        (void)pcops_zero_async(dw, K * o * sizeof(float), s);
        if (dbias) (void)pcops_zero_async(dbias, (size_t)o * sizeof(float), s);
        return pcops_launch_status();
    }
    PCOPS_REQUIRE_PTR(feat); PCOPS_REQUIRE_PTR(idx); PCOPS_REQUIRE_PTR(g); PCOPS_REQUIRE_PTR(dy);
    const int P = b * n, splits = wgrad_splits(b, n, c, k, o);
    if (splits > 1) PCOPS_REQUIRE_PTR(workspace);
    const int chunk = (int)(cdiv(cdiv(P, splits), kBM) * kBM);
    float *ws = static_cast<float *>(workspace);
    float *wdst = splits > 1 ? ws : dw;
    float *bdst = dbias ? (splits > 1 ? ws + (size_t)splits * K * o : dbias) : nullptr;
    const int cblocks = (c + kCB - 1) / kCB;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3(k * cblocks, cdiv(o, kBN), splits), dim3(kThreads), 0, s, P, n, c, k, o,
                       chunk, feat, idx, g, dy, wdst, bdst);
    if (splits > 1) {
        const long long len = (long long)K * o;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(len, kThreads)), dim3(kThreads), 0, s, len, splits, ws, dw);
        if (dbias)
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(o, kThreads)), dim3(kThreads), 0, s, (long long)o, splits,
                               bdst, dbias);
    }
    pcops_note_pipe(0);
    return pcops_launch_status();
}

extern "C" int pcops_spider_conv_dgrad(int b, int n, int c, int k, int t, int o, const float *feat, const int *idx,
                                       const float *g, const float *w, const float *dy, float *dfeat_grouped,
                                       float *dg, pcops_stream_t stream) {
    const int st = check_conv(b, n, c, k, t, o);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(feat); PCOPS_REQUIRE_PTR(idx); PCOPS_REQUIRE_PTR(g); PCOPS_REQUIRE_PTR(w);
    PCOPS_REQUIRE_PTR(dy); PCOPS_REQUIRE_PTR(dg);
    hipLaunchKernelGGL(conv_dgrad_kernel, dim3(cdiv(n, kBM), k, b), dim3(kThreads), 0, as_stream(stream), n, c, k, o,
                       feat, idx, g, w, dy, dfeat_grouped, dg);
    pcops_note_pipe(0);
    return pcops_launch_status();
}

static int check_gn(int b, int n, int c, int groups) {
    PCOPS_REQUIRE_SHAPE(b >= 0 && n > 0 && c > 0);
    PCOPS_REQUIRE_ARG(groups > 0 && c % groups == 0);
    if (c / groups > kThreads || c > 4096) return PCOPS_ERR_UNSUPPORTED;
    if ((long long)b * n * c >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}

extern "C" unsigned long long pcops_group_norm_relu_workspace_bytes(int b, int c) {
    if (b <= 0 || c <= 0) return 0;
    return (unsigned long long)b * 2 * c * sizeof(float);
}

extern "C" int pcops_group_norm_relu_fwd(int b, int n, int c, int groups, float eps, const float *x,
                                         const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                                         pcops_stream_t stream) {
    const int st = check_gn(b, n, c, groups);
    if (st != PCOPS_OK) return st;
    PCOPS_REQUIRE_ARG(eps >= 0.f);
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(x); PCOPS_REQUIRE_PTR(gamma); PCOPS_REQUIRE_PTR(beta); PCOPS_REQUIRE_PTR(y);
    PCOPS_REQUIRE_PTR(mean); PCOPS_REQUIRE_PTR(rstd);
    hipLaunchKernelGGL(gn_fwd_kernel, dim3(groups, b), dim3(kThreads), 0, as_stream(stream), n, c, groups, eps, x, gamma,
                       beta, y, mean, rstd);
    return pcops_launch_status();
}

extern "C" int pcops_group_norm_relu_bwd(int b, int n, int c, int groups, const float *dout, const float *x,
                                         const float *y, const float *gamma, const float *mean, const float *rstd,
                                         float *dx, float *dgamma, float *dbeta, void *workspace,
                                         pcops_stream_t stream) {
    const int st = check_gn(b, n, c, groups);
    if (st != PCOPS_OK) return st;
    PCOPS_REQUIRE_PTR(dgamma); PCOPS_REQUIRE_PTR(dbeta);
    hipStream_t s = as_stream(stream);
    if (b == 0) {
        (void)pcops_zero_async(dgamma, (size_t)c * sizeof(float), s);
        (void)pcops_zero_async(dbeta, (size_t)c * sizeof(float), s);
        return pcops_launch_status();
    }
    PCOPS_REQUIRE_PTR(dout); PCOPS_REQUIRE_PTR(x); PCOPS_REQUIRE_PTR(y); PCOPS_REQUIRE_PTR(gamma);
    PCOPS_REQUIRE_PTR(mean); PCOPS_REQUIRE_PTR(rstd); PCOPS_REQUIRE_PTR(dx); PCOPS_REQUIRE_PTR(workspace);
    float *ws = static_cast<float *>(workspace);
    hipLaunchKernelGGL(gn_bwd_kernel, dim3(groups, b), dim3(kThreads), 0, s, n, c, groups, dout, x, y, gamma, mean, rstd,
                       dx, ws);
    hipLaunchKernelGGL(gn_bwd_final_kernel, dim3(cdiv(c, kThreads)), dim3(kThreads), 0, s, b, c, ws, dgamma, dbeta);
    return pcops_launch_status();
}
