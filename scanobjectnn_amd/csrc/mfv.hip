// mfv.hip -- the two costs of 3DmFV-Net (reference 3DmFV-Net/utils/tf_util.py:578-652, models/3dmfv_net_cls.py:86-102) on gfx950.
//
// 1. The 3DmFV representation (pcops_fv3d_fwd).  points (b, n, 3), a fixed mixture w (K), mu (K, 3), sigma (K, 3) (standard
//    deviations).  Per (point, Gaussian): wp = w N(x; mu, diag sigma^2), Q = wp / sum_k wp, z = (x - mu) / sigma and
//      d_pi = Q - w,   d_mu = Q z,   d_sigma = Q (z^2 - 1);
//    per Gaussian over the points: max, sum of d_pi; max, min, sum of d_mu and of d_sigma per axis -- 20 rows -- scaled by
//    1 / (n sqrt(w)) (d_pi, d_mu) and 1 / (n sqrt(2 w)) (d_sigma), power-normalised sign(x) sqrt|x| and L2-normalised over
//    the Gaussians per (cloud, row).  Nothing of size n K reaches memory: one workgroup takes (cloud, chunk of 512 points),
//    a thread owns Gaussians tid and tid + 256 and keeps their 20 statistics in registers over the chunk, 64 points at a
//    time (their denominators first: four strided partial sums per point added in a fixed order).  Chunk partials go to
//    the workspace and fv_finish_kernel folds them in ascending chunk order, scales, and normalises.
//
// 2. 3-D convolution, k^3 taps with k in {3, 5}, stride 1, SAME, on a cubic grid of R^3 <= 8^3 voxels
//    (pcops_conv3d_fwd / _dgrad / _wgrad).  Activations are VOXEL-MAJOR: x (R^3, b, cin), y (R^3, b, cout); weights
//    (k, k, k, cin, cout) as in the reference.  The b rows of one voxel share one list of in-grid taps, so
//      y[v] = bias + sum_{t in grid at v} x[v + t] w[t]
//    is a chain of dense (b x cin) (cin x cout) products on contiguous rows: no expanded operand, no mask, no gather, and
//    no matrix instruction on a tap that falls outside the grid.  The data gradient is the same kernel on the mirrored,
//    transposed weights (one rearranging launch).  The weight gradient dW[t] = sum_{v: v + t in grid} x[v + t]^T dy[v]
//    runs one workgroup per (tap, 64 cin, 64 cout) over the rows (in-grid voxel, cloud) of that tap, 64 at a time, split
//    over rows where the grid alone leaves the device idle; split partials are added in ascending order.
//
// fp32 MFMA (v_mfma_f32_16x16x4_f32): A[l&15][k=l>>4], B[k=l>>4][l&15], C/D col = l&15, row = 4 (l>>4) + reg.
// Every sum is taken in a fixed order: no float atomics anywhere in this file.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------------ representation
constexpr int kFvRows = 20;
constexpr int kFvChunk = 512;   // points per workgroup
constexpr int kFvTile = 64;     // points per LDS tile
constexpr int kFvMaxK = 512;    // two Gaussians per thread
constexpr int kFvKpt = kFvMaxK / kThreads;

__device__ __forceinline__ float fv_sq(float x, float y, float z, float mx, float my, float mz, float ix, float iy,
                                       float iz, float &zx, float &zy, float &zz) {
    zx = (x - mx) * ix; zy = (y - my) * iy; zz = (z - mz) * iz;
    return fmaf(zz, zz, fmaf(zy, zy, zx * zx));
}

// grid (chunks, b).  ws[cloud][chunk][20][K]
__global__ void __launch_bounds__(kThreads) fv_partial_kernel(int n, int K, const float *__restrict__ pts,
                                                              const float *__restrict__ w, const float *__restrict__ mu,
                                                              const float *__restrict__ sigma, float *__restrict__ ws) {
    __shared__ float sMu[3][kFvMaxK], sInv[3][kFvMaxK], sCoef[kFvMaxK];
    __shared__ float sPt[kFvTile][3], sPart[4][kFvTile], sDen[kFvTile];
    const int tid = threadIdx.x, chunk = blockIdx.x, cloud = blockIdx.y;
    for (int k = tid; k < K; k += kThreads) {
        const float sx = sigma[3 * k], sy = sigma[3 * k + 1], sz = sigma[3 * k + 2];
        sMu[0][k] = mu[3 * k]; sMu[1][k] = mu[3 * k + 1]; sMu[2][k] = mu[3 * k + 2];
        sInv[0][k] = 1.f / sx; sInv[1][k] = 1.f / sy; sInv[2][k] = 1.f / sz;
        sCoef[k] = w[k] / (15.749609945722419f * (sx * sy * sz));      // (2 pi)^(3/2)
    }
    float wk[kFvKpt], st[kFvKpt][kFvRows];
#pragma unroll
    for (int g = 0; g < kFvKpt; ++g) {
        const int k = tid + g * kThreads;
        wk[g] = k < K ? w[k] : 0.f;
#pragma unroll
        for (int r = 0; r < kFvRows; ++r) st[g][r] = 0.f;
        st[g][0] = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            st[g][2 + a] = -INFINITY; st[g][5 + a] = INFINITY;
            st[g][11 + a] = -INFINITY; st[g][14 + a] = INFINITY;
        }
    }
    const int pbeg = chunk * kFvChunk, pend = min(n, pbeg + kFvChunk);
    const float *cp = pts + (size_t)cloud * n * 3;
    for (int p0 = pbeg; p0 < pend; p0 += kFvTile) {
        const int np = min(kFvTile, pend - p0);
        __syncthreads();
        if (tid < kFvTile * 3) sPt[tid / 3][tid % 3] = tid < np * 3 ? cp[(size_t)p0 * 3 + tid] : 0.f;
        __syncthreads();
        {   // denominators: thread (point, part) adds the Gaussians part, part + 4, ... in ascending order
            const int pt = tid & (kFvTile - 1), part = tid >> 6;
            const float x = sPt[pt][0], y = sPt[pt][1], z = sPt[pt][2];
            float s = 0.f, zx, zy, zz;
            for (int k = part; k < K; k += 4) {
                const float q = fv_sq(x, y, z, sMu[0][k], sMu[1][k], sMu[2][k], sInv[0][k], sInv[1][k], sInv[2][k], zx,
                                      zy, zz);
                s += sCoef[k] * expf(-0.5f * q);
            }
            sPart[part][pt] = s;
        }
        __syncthreads();
        if (tid < kFvTile) sDen[tid] = (sPart[0][tid] + sPart[1][tid]) + (sPart[2][tid] + sPart[3][tid]);
        __syncthreads();
#pragma unroll
        for (int g = 0; g < kFvKpt; ++g) {
            const int k = tid + g * kThreads;
            if (k >= K) continue;
            const float mx = sMu[0][k], my = sMu[1][k], mz = sMu[2][k];
            const float ix = sInv[0][k], iy = sInv[1][k], iz = sInv[2][k], cf = sCoef[k];
            for (int p = 0; p < np; ++p) {
                float zc[3];
                const float q = fv_sq(sPt[p][0], sPt[p][1], sPt[p][2], mx, my, mz, ix, iy, iz, zc[0], zc[1], zc[2]);
                const float Q = cf * expf(-0.5f * q) / sDen[p];
                const float dpi = Q - wk[g];
                st[g][0] = fmaxf(st[g][0], dpi);
                st[g][1] += dpi;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float dm = Q * zc[a], ds = Q * (zc[a] * zc[a] - 1.f);
                    st[g][2 + a] = fmaxf(st[g][2 + a], dm);
                    st[g][5 + a] = fminf(st[g][5 + a], dm);
                    st[g][8 + a] += dm;
                    st[g][11 + a] = fmaxf(st[g][11 + a], ds);
                    st[g][14 + a] = fminf(st[g][14 + a], ds);
                    st[g][17 + a] += ds;
                }
            }
        }
    }
    float *out = ws + ((size_t)cloud * gridDim.x + chunk) * kFvRows * K;
#pragma unroll
    for (int g = 0; g < kFvKpt; ++g) {
        const int k = tid + g * kThreads;
        if (k >= K) continue;
#pragma unroll
        for (int r = 0; r < kFvRows; ++r) out[(size_t)r * K + k] = st[g][r];
    }
}

// 0: max, 1: min, 2: sum -- rows d_pi (max, sum), d_mu (max xyz, min xyz, sum xyz), d_sigma (the same)
__device__ __forceinline__ int fv_row_kind(int row) {
    if (row < 2) return row == 0 ? 0 : 2;
    return ((row - 2) % 9) / 3;
}

// grid (20, b): one (cloud, row); fv (b, 20, K), or (K, b, 20) with voxel_major
__global__ void __launch_bounds__(kThreads) fv_finish_kernel(int b, int n, int K, int chunks, int voxel_major,
                                                             const float *__restrict__ w, const float *__restrict__ ws,
                                                             float *__restrict__ fv) {
    __shared__ float red[kThreads];
    const int tid = threadIdx.x, row = blockIdx.x, cloud = blockIdx.y, kind = fv_row_kind(row);
    float val[kFvKpt], ss = 0.f;
#pragma unroll
    for (int g = 0; g < kFvKpt; ++g) {
        const int k = tid + g * kThreads;
        val[g] = 0.f;
        if (k >= K) continue;
        const float *src = ws + ((size_t)cloud * chunks * kFvRows + row) * K + k;
        float s = src[0];
        for (int c = 1; c < chunks; ++c) {
            const float v = src[(size_t)c * kFvRows * K];
            s = kind == 0 ? fmaxf(s, v) : kind == 1 ? fminf(s, v) : s + v;
        }
        const float wv = w[k];
        if (row < 2) s = s / (sqrtf(wv) * (float)n);
        else if (row < 11) s = s * (1.f / ((float)n * sqrtf(wv)));
        else s = s * (1.f / ((float)n * sqrtf(2.f * wv)));
        const float pw = sqrtf(fabsf(s));
        val[g] = s > 0.f ? pw : (s < 0.f ? -pw : 0.f);
        ss = fmaf(val[g], val[g], ss);
    }
    red[tid] = ss;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float inv = 1.f / sqrtf(fmaxf(red[0], 1e-12f));
#pragma unroll
    for (int g = 0; g < kFvKpt; ++g) {
        const int k = tid + g * kThreads;
        if (k >= K) continue;
        const size_t o = voxel_major ? ((size_t)k * b + cloud) * kFvRows + row : ((size_t)cloud * kFvRows + row) * K + k;
        fv[o] = val[g] * inv;
    }
}

int check_fv(int b, int n, int k) {
    PCOPS_REQUIRE_SHAPE(b >= 0 && n >= 1 && k >= 1);
    if (k > kFvMaxK || b > 65535) return PCOPS_ERR_UNSUPPORTED;
    if ((long long)b * n * 3 >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    if ((long long)b * cdiv(n, kFvChunk) * kFvRows * k >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}

// --------------------------------------------------------------------------------------------------------- convolution
constexpr int kBM = 64;   // rows per tile
constexpr int kBN = 64;   // output columns per tile
constexpr int kKB = 32;   // input channels per step
constexpr int kMaxR = 8;

// in-grid range of one axis: voxel coordinates [lo, hi) whose neighbour at offset d lies in [0, R)
__device__ __host__ __forceinline__ int ax_lo(int d) { return d < 0 ? -d : 0; }
__device__ __host__ __forceinline__ int ax_hi(int R, int d) { return d > 0 ? R - d : R; }

// grid (ceil(b / 64), ceil(cout / 64), R^3); 4 waves, each a 32 x 32 quarter of the 64 x 64 output tile
__global__ void __launch_bounds__(kThreads) conv3d_fwd_kernel(int B, int R, int ks, int Cin, int Cout,
                                                              const float *__restrict__ X, const float *__restrict__ W,
                                                              const float *__restrict__ bias, float *__restrict__ Y) {
    __shared__ float As[kBM][kKB + 1];   // As[row][kk]
    __shared__ float Bs[kKB][kBN + 4];   // Bs[kk][col]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * kBM, col0 = blockIdx.y * kBN, v = blockIdx.z;
    const int vc = v % R, vb = (v / R) % R, va = v / (R * R), h = ks / 2;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const bool live = row0 + wr < B && col0 + wc < Cout;     // wave-uniform: a quarter with no row or no column idles
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ta = max(0, h - va); ta < min(ks, R + h - va); ++ta)
        for (int tb = max(0, h - vb); tb < min(ks, R + h - vb); ++tb)
            for (int tc = max(0, h - vc); tc < min(ks, R + h - vc); ++tc) {
                const int tap = (ta * ks + tb) * ks + tc;
                const int u = ((va + ta - h) * R + (vb + tb - h)) * R + (vc + tc - h);
                const float *xr = X + (size_t)u * B * Cin;
                const float *wt = W + (size_t)tap * Cin * Cout;
                for (int c0 = 0; c0 < Cin; c0 += kKB) {
                    __syncthreads();
                    for (int e = tid; e < kBM * kKB; e += kThreads) {
                        const int r = e >> 5, kk = e & 31;
                        As[r][kk] = (row0 + r < B && c0 + kk < Cin) ? xr[(size_t)(row0 + r) * Cin + c0 + kk] : 0.f;
                    }
                    for (int e = tid; e < kKB * kBN; e += kThreads) {
                        const int kk = e >> 6, cl = e & 63;
                        Bs[kk][cl] = (c0 + kk < Cin && col0 + cl < Cout) ? wt[(size_t)(c0 + kk) * Cout + col0 + cl] : 0.f;
                    }
                    __syncthreads();
                    if (live) {
#pragma unroll
                        for (int s = 0; s < kKB / 4; ++s) {
                            const int kk = s * 4 + (lane >> 4);
                            float a[2], bv[2];
#pragma unroll
                            for (int i = 0; i < 2; ++i) a[i] = As[wr + i * 16 + (lane & 15)][kk];
#pragma unroll
                            for (int jj = 0; jj < 2; ++jj) bv[jj] = Bs[kk][wc + jj * 16 + (lane & 15)];
#pragma unroll
                            for (int i = 0; i < 2; ++i)
#pragma unroll
                                for (int jj = 0; jj < 2; ++jj)
                                    acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[jj], acc[i][jj], 0, 0, 0);
                        }
                    }
                }
            }
    float *yr = Y + (size_t)v * B * Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int col = col0 + wc + jj * 16 + (lane & 15);
            if (col >= Cout) continue;
            const float bb = bias ? bias[col] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = row0 + wr + i * 16 + (lane >> 4) * 4 + q;
                if (row < B) yr[(size_t)row * Cout + col] = acc[i][jj][q] + bb;
            }
        }
}

// wt[T - 1 - t][o][c] = w[t][c][o]: the mirrored taps, each tap's matrix transposed
__global__ void __launch_bounds__(kThreads) conv3d_flip_kernel(int T, int Cin, int Cout, const float *__restrict__ w,
                                                               float *__restrict__ wt) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)T * Cin * Cout) return;
    const int c = (int)(i % Cin), o = (int)((i / Cin) % Cout), t = (int)(i / ((long long)Cin * Cout));
    wt[i] = w[((size_t)(T - 1 - t) * Cin + c) * Cout + o];
}

// grid (k^3 ceil(cin / 64), ceil(cout / 64), splits).  The rows of tap t are (in-grid voxel index, cloud) pairs in ascending
// order; split s takes the 64-row steps [s chunk, (s + 1) chunk) of its tap, chunk = ceil(steps / splits).  With splits > 1
// the tile goes to ws[s][k^3 cin cout] (db to ws_db[s][cout]) and wgrad_reduce_kernel adds the splits in ascending order.
// The workgroups of the centre tap (every voxel in grid) and cin tile 0 also take the column sums of dY (db).
__global__ void __launch_bounds__(kThreads) conv3d_wgrad_kernel(int B, int R, int ks, int Cin, int Cout,
                                                                const float *__restrict__ X,
                                                                const float *__restrict__ dY, float *__restrict__ dw,
                                                                float *__restrict__ db) {
    __shared__ float At[kBM][kBN + 4];   // At[p][cin]
    __shared__ float Ds[kBM][kBN + 4];   // Ds[p][cout]
    __shared__ int sX[kBM], sY[kBM];     // global row of x / dy, -1 past the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctiles = (Cin + kBM - 1) / kBM;
    const int tap = blockIdx.x / ctiles, ci0 = (blockIdx.x - tap * ctiles) * kBM;
    const int co0 = blockIdx.y * kBN, split = blockIdx.z, splits = gridDim.z, h = ks / 2;
    const int da = tap / (ks * ks) - h, dbb = (tap / ks) % ks - h, dc = tap % ks - h;
    const int la = ax_lo(da), lb = ax_lo(dbb), lc = ax_lo(dc);
    const int na = ax_hi(R, da) - la, nb = ax_hi(R, dbb) - lb, nc = ax_hi(R, dc) - lc;
    const int rows = (na > 0 && nb > 0 && nc > 0) ? na * nb * nc * B : 0;
    const int steps = (rows + kBM - 1) / kBM, chunk = (steps + splits - 1) / splits;
    const int sbeg = split * chunk, send = min(steps, sbeg + chunk);
    const bool do_db = db != nullptr && tap == (ks * ks * ks) / 2 && ci0 == 0;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const bool live = ci0 + wr < Cin && co0 + wc < Cout;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;

    for (int st = sbeg; st < send; ++st) {
        __syncthreads();
        if (tid < kBM) {
            const int q = st * kBM + tid;
            int xr = -1, yr = -1;
            if (q < rows) {
                const int vi = q / B, bb = q - vi * B;
                const int ic = vi % nc, ib = (vi / nc) % nb, ia = vi / (nc * nb);
                const int v = ((la + ia) * R + (lb + ib)) * R + (lc + ic);
                const int u = ((la + ia + da) * R + (lb + ib + dbb)) * R + (lc + ic + dc);
                xr = u * B + bb;
                yr = v * B + bb;
            }
            sX[tid] = xr;
            sY[tid] = yr;
        }
        __syncthreads();
        for (int e = tid; e < kBM * kBN; e += kThreads) {
            const int r = e >> 6, cl = e & 63;
            At[r][cl] = (sX[r] >= 0 && ci0 + cl < Cin) ? X[(size_t)sX[r] * Cin + ci0 + cl] : 0.f;
            Ds[r][cl] = (sY[r] >= 0 && co0 + cl < Cout) ? dY[(size_t)sY[r] * Cout + co0 + cl] : 0.f;
        }
        __syncthreads();
        if (do_db && tid < kBN) {
            for (int r = 0; r < kBM; ++r) dbs += Ds[r][tid];
        }
        if (live) {
#pragma unroll 4
            for (int s = 0; s < kBM / 4; ++s) {
                const int pr = s * 4 + (lane >> 4);
                float a[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = At[pr][wr + i * 16 + (lane & 15)];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) bv[jj] = Ds[pr][wc + jj * 16 + (lane & 15)];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[jj], acc[i][jj], 0, 0, 0);
            }
        }
    }
    const size_t len = (size_t)ks * ks * ks * Cin * Cout;
    float *out = (splits > 1 ? dw + (size_t)split * len : dw) + (size_t)tap * Cin * Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int col = co0 + wc + jj * 16 + (lane & 15);
            if (col >= Cout) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = ci0 + wr + i * 16 + (lane >> 4) * 4 + q;
                if (ci < Cin) out[(size_t)ci * Cout + col] = acc[i][jj][q];
            }
        }
    if (do_db && tid < kBN && co0 + tid < Cout) db[(size_t)(splits > 1 ? split : 0) * Cout + co0 + tid] = dbs;
}

__global__ void wgrad_reduce_kernel(long long len, int splits, const float *__restrict__ ws, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= len) return;
    float s = 0.f;
    for (int q = 0; q < splits; ++q) s += ws[(size_t)q * len + i];
    out[i] = s;
}

int check_conv3d(int b, int r, int k, int cin, int cout) {
    PCOPS_REQUIRE_SHAPE(b >= 0 && r >= 1 && cin >= 1 && cout >= 1);
    if (r > kMaxR || (k != 3 && k != 5)) return PCOPS_ERR_UNSUPPORTED;
    if (cin % 16 != 0 || cout % 16 != 0 || cin > 512 || cout > 512) return PCOPS_ERR_UNSUPPORTED;
    if ((long long)r * r * r * b * std::max(cin, cout) >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    if (cdiv(b, kBM) > 65535) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}

// split count of the weight gradient: a power of two, doubled while the grid stays within 1024 workgroups and every split of
// the centre tap still holds a 64-row step; at most 16
int conv3d_splits(int b, int r, int k, int cin, int cout) {
    const long long nwg = (long long)k * k * k * cdiv(cin, kBM) * cdiv(cout, kBN);
    const long long steps = cdiv((long long)r * r * r * b, kBM);
    int s = 1;
    while (s < 16 && nwg * s * 2 <= 1024 && s * 2 <= steps) s *= 2;
    return s;
}

int launch_conv3d_fwd(int b, int r, int k, int cin, int cout, const float *x, const float *w, const float *bias, float *y,
                      hipStream_t s) {
    hipLaunchKernelGGL(conv3d_fwd_kernel, dim3(cdiv(b, kBM), cdiv(cout, kBN), r * r * r), dim3(kThreads), 0, s, b, r, k,
                       cin, cout, x, w, bias, y);
    pcops_note_pipe(0);
    return pcops_launch_status();
}

}  // namespace

extern "C" unsigned long long pcops_fv3d_workspace_bytes(int b, int n, int k) {
    if (check_fv(b, n, k) != PCOPS_OK || b == 0) return 0;
    return (unsigned long long)b * cdiv(n, kFvChunk) * kFvRows * k * sizeof(float);
}

extern "C" int pcops_fv3d_fwd(int b, int n, int k, int voxel_major, const float *points, const float *w, const float *mu,
                              const float *sigma, float *fv, void *workspace, pcops_stream_t stream) {
    const int st = check_fv(b, n, k);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(points); PCOPS_REQUIRE_PTR(w); PCOPS_REQUIRE_PTR(mu); PCOPS_REQUIRE_PTR(sigma);
    PCOPS_REQUIRE_PTR(fv); PCOPS_REQUIRE_PTR(workspace);
    hipStream_t s = as_stream(stream);
    const int chunks = (int)cdiv(n, kFvChunk);
    float *ws = static_cast<float *>(workspace);
    hipLaunchKernelGGL(fv_partial_kernel, dim3(chunks, b), dim3(kThreads), 0, s, n, k, points, w, mu, sigma, ws);
    hipLaunchKernelGGL(fv_finish_kernel, dim3(kFvRows, b), dim3(kThreads), 0, s, b, n, k, chunks, voxel_major ? 1 : 0, w,
                       ws, fv);
    return pcops_launch_status();
}

extern "C" int pcops_conv3d_fwd(int b, int r, int k, int cin, int cout, const float *x, const float *w, const float *bias,
                                float *y, pcops_stream_t stream) {
    const int st = check_conv3d(b, r, k, cin, cout);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(x); PCOPS_REQUIRE_PTR(w); PCOPS_REQUIRE_PTR(y);
    return launch_conv3d_fwd(b, r, k, cin, cout, x, w, bias, y, as_stream(stream));
}

extern "C" unsigned long long pcops_conv3d_dgrad_workspace_bytes(int b, int r, int k, int cin, int cout) {
    if (check_conv3d(b, r, k, cin, cout) != PCOPS_OK || b == 0) return 0;
    return (unsigned long long)k * k * k * cin * cout * sizeof(float);
}

extern "C" int pcops_conv3d_dgrad(int b, int r, int k, int cin, int cout, const float *w, const float *dy, float *dx,
                                  void *workspace, pcops_stream_t stream) {
    const int st = check_conv3d(b, r, k, cin, cout);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(w); PCOPS_REQUIRE_PTR(dy); PCOPS_REQUIRE_PTR(dx); PCOPS_REQUIRE_PTR(workspace);
    hipStream_t s = as_stream(stream);
    float *wt = static_cast<float *>(workspace);
    const long long len = (long long)k * k * k * cin * cout;
    hipLaunchKernelGGL(conv3d_flip_kernel, dim3(cdiv(len, kThreads)), dim3(kThreads), 0, s, k * k * k, cin, cout, w, wt);
    return launch_conv3d_fwd(b, r, k, cout, cin, dy, wt, nullptr, dx, s);
}

extern "C" int pcops_conv3d_wgrad_splits(int b, int r, int k, int cin, int cout) {
    if (check_conv3d(b, r, k, cin, cout) != PCOPS_OK || b == 0) return 0;
    return conv3d_splits(b, r, k, cin, cout);
}

extern "C" unsigned long long pcops_conv3d_wgrad_workspace_bytes(int b, int r, int k, int cin, int cout) {
    if (check_conv3d(b, r, k, cin, cout) != PCOPS_OK || b == 0) return 0;
    const int s = conv3d_splits(b, r, k, cin, cout);
    if (s <= 1) return 0;
    return (unsigned long long)s * ((unsigned long long)k * k * k * cin * cout + cout) * sizeof(float);
}

extern "C" int pcops_conv3d_wgrad(int b, int r, int k, int cin, int cout, const float *x, const float *dy, float *dw,
                                  float *dbias, void *workspace, pcops_stream_t stream) {
    const int st = check_conv3d(b, r, k, cin, cout);
    if (st != PCOPS_OK) return st;
    PCOPS_REQUIRE_PTR(dw);
    hipStream_t s = as_stream(stream);
    const size_t len = (size_t)k * k * k * cin * cout;
    if (b == 0) {
        (void)pcops_zero_async(dw, len * sizeof(float), s);
        if (dbias) (void)pcops_zero_async(dbias, (size_t)cout * sizeof(float), s);
        return pcops_launch_status();
    }
    PCOPS_REQUIRE_PTR(x); PCOPS_REQUIRE_PTR(dy);
    const int splits = conv3d_splits(b, r, k, cin, cout);
    if (splits > 1) PCOPS_REQUIRE_PTR(workspace);
    float *ws = static_cast<float *>(workspace);
    float *wdst = splits > 1 ? ws : dw;
    float *bdst = dbias ? (splits > 1 ? ws + (size_t)splits * len : dbias) : nullptr;
    hipLaunchKernelGGL(conv3d_wgrad_kernel, dim3(k * k * k * cdiv(cin, kBM), cdiv(cout, kBN), splits), dim3(kThreads), 0, s,
                       b, r, k, cin, cout, x, dy, wdst, bdst);
    if (splits > 1) {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long long)len, kThreads)), dim3(kThreads), 0, s, (long long)len,
                           splits, ws, dw);
        if (dbias)
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(cout, kThreads)), dim3(kThreads), 0, s, (long long)cout, splits,
                               bdst, dbias);
    }
    pcops_note_pipe(0);
    return pcops_launch_status();
}
