// cloudpoint.hip -- first conv of PointNet's segmentation heads on concat([per-point 64 | per-cloud 1024]) without the
// concatenation and without the (rows, c) product in memory (reference pointnet/models/pointnet_seg.py:81-88,
// pointnet_partseg.py:66-73) on gfx950.
//
//   forward   Y[r][:] = X[r][:] Wx + Ctr[r / n][:]                 X (b n, 64), Wx (64, c), Ctr (b, c), Y (b n, c)
//             stats_partial[P][2][c] = per workgroup sums of (y - pivot) and (y - pivot)^2 over its rows
//   backward  D = p G + q Y + t (registers and LDS only),  dX = D Wx^T,  dWx = X^T D,  dCtr[cloud] = sum of the cloud's rows of D
//
// Every product runs on v_mfma_f32_16x16x4_f32 with exact fp32 operands.  Lane maps of that instruction (lane l, g = l >> 4,
// l15 = l & 15): A[row = l15][kk = g], B[kk = g][col = l15], C/D row = 4 g + reg, col = l15.  As in tnet.hip a lane loads its
// row of X (or of G and Y) as four 16-byte pieces, columns 16 jj + 4 g + (0..3), and step (jj, e) multiplies column
// 16 jj + 4 g + e: coalesced 16-byte loads, no shuffle.
// Channels are walked in chunks of 64.  FORWARD: a workgroup owns 128 points of ONE cloud (two 16-point tiles per wave, their
// rows of X held in registers for all chunks) and stages Wx[:, chunk] in LDS, row stride 68 words, two buffers so that one
// barrier per chunk is enough: a B-operand read is S[k][l15 + 16 t] with k differing by 4 between the two lane groups of a
// 32-lane half, 4 x 68 = 272 = 16 (mod 32) -- 32 lanes on 32 banks; one read feeds both tiles of the wave.
// BACKWARD: grid (splits, b); a split of a cloud walks its points 64 per step, and per step the channel chunks of the pass.
// Per (step, chunk) a wave forms D for its 16 rows from G, Y (loaded one chunk ahead, under the products of the chunk before)
// and the p / q / t kept in LDS, leaves it in LDS (Ds, stride 80: rows p and p + 1 of the transposed use X^T D are 16 banks
// apart, as in tnet.hip), adds D Wx^T to its rows of dX against the
// chunk of Wx staged TRANSPOSED (stride 68, the same reads as the forward), and wave w adds rows 16 w .. 16 w + 15 of X^T D to
// the accumulators it keeps for every chunk of the pass (16 registers per chunk: a pass is at most 512 channels = 128
// registers; wider layers take a second pass whose dX adds to the first's).  dCtr: thread (wave, lane) adds channel `lane` of
// the 16 rows 16 wave .. of Ds (64 consecutive words per read), the four waves' sums are added at the end.
// Every sum is taken in a fixed order; there is no float atomic in this file.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kK = 64;            // per-point width
constexpr int kCW = 64;           // channel chunk
constexpr int kLd = 68;           // LDS row stride of a 64 x 64 weight chunk
constexpr int kTileLd = 80;       // LDS row stride of the backward's point tiles
constexpr int kThreads = 256;     // 4 waves
constexpr int kWaves = kThreads / kWave;
constexpr int kFwdPoints = 128;   // forward: points per workgroup (two 16-point tiles per wave)
constexpr int kPT = 64;           // backward: points per step (one 16-point tile per wave); a split is a whole number of them
constexpr int kSplitCap = 16;     // backward: splits per cloud (a power of two)
constexpr int kTargetWGs = 512;
constexpr int kPassChunks = 8;    // backward: chunks per pass (the dWx accumulators of a pass live in registers)


// row p of a (n, 64) cloud as this lane's four 16-byte pieces: a[jj] = row[16 jj + 4 g .. + 3]; zeros past n
__device__ __forceinline__ void load_row(const float *__restrict__ cloud, int p, int n, int g, f32x4 a[4]) {
    if (p < n) {
        const f32x4 *r = reinterpret_cast<const f32x4 *>(cloud + (size_t)p * kK);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) a[jj] = r[4 * jj + g];
    } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) a[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// Wx[:, cb .. cb + 63] (row stride c) -> LDS [64][68]
__device__ __forceinline__ void stage_chunk(const float *__restrict__ Wx, int c, int cb, float *S) {
    for (int e = threadIdx.x; e < kK * kCW / 4; e += kThreads) {
        const int i = e >> 4, j = (e & 15) * 4;
        *reinterpret_cast<f32x4 *>(S + i * kLd + j) = *reinterpret_cast<const f32x4 *>(Wx + (size_t)i * c + cb + j);
    }
}

// the same chunk transposed: S[ch][k] = Wx[k][cb + ch]
__device__ __forceinline__ void stage_chunk_transposed(const float *__restrict__ Wx, int c, int cb, float *S) {
    for (int e = threadIdx.x; e < kK * kCW; e += kThreads) S[(e & 63) * kLd + (e >> 6)] = Wx[(size_t)(e >> 6) * c + cb + (e & 63)];
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (ceil(n / 128), b): all points of a workgroup belong to cloud blockIdx.y; partial row = cloud gridDim.x + blockIdx.x
template <bool STATS>
__global__ void __launch_bounds__(kThreads) cloud_point_fwd_kernel(int n, int c, const float *__restrict__ X,
                                                                   const float *__restrict__ Wx, const float *__restrict__ Ctr,
                                                                   float *__restrict__ Y, float *__restrict__ stats,
                                                                   const float *__restrict__ pivot) {
    __shared__ __attribute__((aligned(16))) float Ws[2][kK * kLd];
    __shared__ float red[2][kWaves][2][kCW];
    const size_t cloud = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const int p0 = blockIdx.x * kFwdPoints + wave * 32;
    const float *Xc = X + cloud * n * kK;
    float *Yc = Y + cloud * n * c;
    const float *ctr = Ctr + cloud * c;
    f32x4 a[2][4];
    load_row(Xc, p0 + l15, n, g, a[0]);
    load_row(Xc, p0 + 16 + l15, n, g, a[1]);
    const int nch = c / kCW;
    stage_chunk(Wx, c, 0, Ws[0]);
    __syncthreads();
    for (int j = 0; j < nch; ++j) {
        if (j + 1 < nch) stage_chunk(Wx, c, (j + 1) * kCW, Ws[(j + 1) & 1]);
        const float *M = Ws[j & 1];
        f32x4 acc[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *row = M + (16 * jj + 4 * g + e) * kLd + l15;
                float bv[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) bv[t] = row[16 * t];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][jj][e], bv[t], acc[u][t], 0, 0, 0);
            }
        }
        const int cb = j * kCW;
        float cv[4], pv[4], s1[4], s2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            cv[t] = ctr[cb + 16 * t + l15];
            pv[t] = (STATS && pivot != nullptr) ? pivot[cb + 16 * t + l15] : 0.f;
            s1[t] = s2[t] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = p0 + 16 * u + 4 * g + r;
                if (p >= n) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float y = acc[u][t][r] + cv[t];
                    Yc[(size_t)p * c + cb + 16 * t + l15] = y;
                    if constexpr (STATS) {
                        const float d = y - pv[t];
                        s1[t] += d;
                        s2[t] = fmaf(d, d, s2[t]);
                    }
                }
            }
        if constexpr (STATS) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s1[t] += __shfl_xor(s1[t], 16);
                s1[t] += __shfl_xor(s1[t], 32);
                s2[t] += __shfl_xor(s2[t], 16);
                s2[t] += __shfl_xor(s2[t], 32);
                if (g == 0) {
                    red[j & 1][wave][0][16 * t + l15] = s1[t];
                    red[j & 1][wave][1][16 * t + l15] = s2[t];
                }
            }
        }
        __syncthreads();
        if constexpr (STATS) {
            if (threadIdx.x < 2 * kCW) {
                const int which = threadIdx.x >> 6, ch = threadIdx.x & 63;
                const float v = ((red[j & 1][0][which][ch] + red[j & 1][1][which][ch]) + red[j & 1][2][which][ch]) +
                                red[j & 1][3][which][ch];
                stats[((cloud * gridDim.x + blockIdx.x) * 2 + which) * c + cb + ch] = v;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// grid (splits, b).  Split s of cloud `cloud` takes the points [s chunk, (s + 1) chunk) below n; the pass covers the NCH
// channel chunks from c0.  dstW: dWx itself (one part) or the workspace [parts][64][c], part = cloud splits + s; dstC: dCtr
// itself (one split per cloud) or the workspace [parts][c].  A split that holds no point stores zeros.  accumulate: this is
// not the first pass, dX += .
template <int NCH, bool DX>
__global__ void __launch_bounds__(kThreads) cloud_point_bwd_kernel(int n, int c, int c0, int chunk, int accumulate,
                                                                   const float *__restrict__ G, const float *__restrict__ Y,
                                                                   const float *__restrict__ pv, const float *__restrict__ qv,
                                                                   const float *__restrict__ tv, const float *__restrict__ X,
                                                                   const float *__restrict__ Wx, float *__restrict__ dX,
                                                                   float *__restrict__ dstW, float *__restrict__ dstC) {
    __shared__ __attribute__((aligned(16))) float Xs[kPT * kTileLd];
    __shared__ __attribute__((aligned(16))) float Ds[kPT * kTileLd];
    __shared__ __attribute__((aligned(16))) float Wt[DX ? kCW * kLd : 4];
    __shared__ __attribute__((aligned(16))) float pqt[3][NCH * kCW];
    static_assert(kWaves * NCH * kCW <= kPT * kTileLd, "the dCtr reduction reuses Ds");
    const size_t cloud = blockIdx.y;
    const size_t part = cloud * gridDim.x + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const int pbeg = (int)min((long long)blockIdx.x * chunk, (long long)n), pend = (int)min((long long)pbeg + chunk, (long long)n);
    for (int e = threadIdx.x; e < NCH * kCW; e += kThreads) {
        pqt[0][e] = pv[c0 + e];
        pqt[1][e] = qv[c0 + e];
        pqt[2][e] = tv[c0 + e];
    }
    __syncthreads();
    const float *Xc = X + cloud * n * kK;
    const float *Gc = G + cloud * n * c, *Yc = Y + cloud * n * c;
    f32x4 accW[NCH][4];
    float accC[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        accC[j] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) accW[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 gv[4], yv[4];
    auto load_gy = [&](int row, int cb) {
        if (row >= pend) return;
        const f32x4 *gr = reinterpret_cast<const f32x4 *>(Gc + (size_t)row * c + cb);
        const f32x4 *yr = reinterpret_cast<const f32x4 *>(Yc + (size_t)row * c + cb);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            gv[jj] = gr[4 * jj + g];
            yv[jj] = yr[4 * jj + g];
        }
    };
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) gv[jj] = yv[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    load_gy(pbeg + 16 * wave + l15, c0);
    for (int p0 = pbeg; p0 < pend; p0 += kPT) {
        const int pw = p0 + 16 * wave, prow = pw + l15;
        {
            f32x4 xr[4];
            load_row(Xc, prow, pend, g, xr);
            float *xs = Xs + (16 * wave + l15) * kTileLd + 4 * g;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) *reinterpret_cast<f32x4 *>(xs + 16 * jj) = xr[jj];
        }
        f32x4 accX[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) accX[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int cb = c0 + j * kCW;
            if constexpr (DX) stage_chunk_transposed(Wx, c, cb, Wt);
            f32x4 d[4];
            if (prow < pend) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int o = j * kCW + 16 * jj + 4 * g;
                    const f32x4 pp = *reinterpret_cast<const f32x4 *>(&pqt[0][o]), qq = *reinterpret_cast<const f32x4 *>(&pqt[1][o]),
                             tt = *reinterpret_cast<const f32x4 *>(&pqt[2][o]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[jj][e] = fmaf(pp[e], gv[jj][e], fmaf(qq[e], yv[jj][e], tt[e]));
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) d[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float *ds = Ds + (16 * wave + l15) * kTileLd + 4 * g;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) *reinterpret_cast<f32x4 *>(ds + 16 * jj) = d[jj];
            __syncthreads();
            // the next chunk's (or the next step's first chunk's) rows of G and Y are on their way under the products
            if (j + 1 < NCH) load_gy(prow, cb + kCW);
            else if (p0 + kPT < pend) load_gy(prow + kPT, c0);
            if constexpr (DX) {
                // dX rows of this wave += D[16 rows][chunk] Wx[:, chunk]^T: B[kk = ch][col = k] = Wt[ch][k]
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float *row = Wt + (16 * jj + 4 * g + e) * kLd + l15;
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            accX[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[jj][e], row[16 * t], accX[t], 0, 0, 0);
                    }
                }
            }
            // dWx[i = 16 w + l15 as A row][ch]: A[row = i][kk = p] = Xs[p][i], B[kk = p][col = ch] = Ds[p][ch]
#pragma unroll 4
            for (int s = 0; s < kPT / 4; ++s) {
                const int pl = 4 * s + g;
                const float av = Xs[pl * kTileLd + 16 * wave + l15];
                const float *drow = Ds + pl * kTileLd + l15;
#pragma unroll
                for (int t = 0; t < 4; ++t) accW[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, drow[16 * t], accW[j][t], 0, 0, 0);
            }
            {
                float sum = accC[j];
#pragma unroll
                for (int i = 0; i < 16; ++i) sum += Ds[(16 * wave + i) * kTileLd + lane];
                accC[j] = sum;
            }
            __syncthreads();
        }
        if constexpr (DX) {
            float *dXc = dX + cloud * n * kK;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = pw + 4 * g + r;
                if (p >= pend) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float *o = dXc + (size_t)p * kK + 16 * t + l15;
                    *o = accumulate ? *o + accX[t][r] : accX[t][r];
                }
            }
        }
    }
    float *ow = dstW + part * kK * c + c0;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) ow[(size_t)(16 * wave + 4 * g + r) * c + j * kCW + 16 * t + l15] = accW[j][t][r];
#pragma unroll
    for (int j = 0; j < NCH; ++j) Ds[wave * NCH * kCW + j * kCW + lane] = accC[j];
    __syncthreads();
    for (int e = threadIdx.x; e < NCH * kCW; e += kThreads)
        dstC[part * c + c0 + e] = ((Ds[e] + Ds[NCH * kCW + e]) + Ds[2 * NCH * kCW + e]) + Ds[3 * NCH * kCW + e];
}

// dWx[e] = ws[0][e] + ws[1][e] + ... : a workgroup owns 64 neighbouring 16-byte elements (len4 = 64 c / 4 is a multiple of 64);
// thread (zq = wave, lane) adds the parts of quarter zq in ascending order, the four quarter sums are added in ascending order
__global__ void __launch_bounds__(kThreads) cloud_point_reduce_w_kernel(int parts, long long len4, const float *__restrict__ ws,
                                                                        float *__restrict__ dWx) {
    __shared__ f32x4 sh[kWaves][64];
    const int lane = threadIdx.x & 63, zq = threadIdx.x >> 6;
    const long long e4 = (long long)blockIdx.x * 64 + lane;
    const int per = (parts + kWaves - 1) / kWaves, zbeg = min(zq * per, parts), zend = min(zbeg + per, parts);
    const f32x4 *src = reinterpret_cast<const f32x4 *>(ws) + e4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int z = zbeg; z < zend; ++z) v += src[(size_t)z * len4];
    sh[zq][lane] = v;
    __syncthreads();
    if (zq == 0) reinterpret_cast<f32x4 *>(dWx)[e4] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// dCtr[cloud][ch] = ws[cloud][0][ch] + ws[cloud][1][ch] + ... in ascending order
__global__ void __launch_bounds__(kThreads) cloud_point_reduce_c_kernel(int splits, int c, long long total,
                                                                        const float *__restrict__ ws, float *__restrict__ dCtr) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long long cloud = i / c;
    const int ch = (int)(i - cloud * c);
    const float *src = ws + cloud * splits * c + ch;
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += src[(size_t)z * c];
    dCtr[i] = v;
}

bool supported(int b, int n, int k, int c) {
    return k == kK && c % kCW == 0 && c >= 64 && c <= 1024 && b >= 1 && b <= 65535 && n >= 1 &&
           (long long)b * n * c < (1ll << 31);
}

// the largest power of two up to the cap that leaves every split at least one 64-point step and stops once the grid has
// kTargetWGs workgroups
int bwd_splits(int b, int n) {
    const long long tiles = (n + kPT - 1) / kPT;
    long long want = std::min<long long>((kTargetWGs + b - 1) / b, tiles);
    want = std::min<long long>(want, kSplitCap);
    int s = 1;
    while (2 * s <= want) s *= 2;
    return s;
}

int bwd_chunk(int n, int splits) {
    const int per = (n + splits - 1) / splits;
    return (per + kPT - 1) / kPT * kPT;
}

template <int NCH>
void launch_bwd_pass(int b, int n, int c, int c0, int splits, int chunk, const float *G, const float *Y, const float *p,
                     const float *q, const float *t, const float *X, const float *Wx, float *dX, float *dstW, float *dstC,
                     hipStream_t hs) {
    if (dX)
        hipLaunchKernelGGL((cloud_point_bwd_kernel<NCH, true>), dim3(splits, b), dim3(kThreads), 0, hs, n, c, c0, chunk,
                           c0 > 0 ? 1 : 0, G, Y, p, q, t, X, Wx, dX, dstW, dstC);
    else
        hipLaunchKernelGGL((cloud_point_bwd_kernel<NCH, false>), dim3(splits, b), dim3(kThreads), 0, hs, n, c, c0, chunk, 0, G,
                           Y, p, q, t, X, Wx, dX, dstW, dstC);
}

}  // namespace

extern "C" int pcops_cloud_point_supported(int b, int n, int k, int c) { return supported(b, n, k, c) ? 1 : 0; }

extern "C" int pcops_cloud_point_rows(int b, int n) {
    if (b < 1 || n < 1) return 0;
    return (int)std::min<long long>((long long)b * ((n + kFwdPoints - 1) / kFwdPoints), 0x7fffffff);
}

extern "C" int pcops_cloud_point_bwd_parts(int b, int n, int c) { return supported(b, n, kK, c) ? b * bwd_splits(b, n) : 0; }

extern "C" unsigned long long pcops_cloud_point_bwd_ws(int b, int n, int k, int c) {
    if (!supported(b, n, k, c)) return 0;
    const int splits = bwd_splits(b, n);
    const unsigned long long parts = (unsigned long long)b * splits;
    return ((parts > 1 ? parts * kK * c : 0) + (splits > 1 ? parts * c : 0)) * sizeof(float);
}

extern "C" int pcops_cloud_point_fwd(int b, int n, int k, int c, const float *X, const float *Wx, const float *Ctr, float *Y,
                                     float *stats_partial, const float *stat_pivot, pcops_stream_t stream) {
    if (!supported(b, n, k, c)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(Wx); PCOPS_REQUIRE_PTR(Ctr); PCOPS_REQUIRE_PTR(Y);
    const dim3 grid(cdiv(n, kFwdPoints), b);
    if (stats_partial)
        hipLaunchKernelGGL(cloud_point_fwd_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), n, c, X, Wx, Ctr, Y,
                           stats_partial, stat_pivot);
    else
        hipLaunchKernelGGL(cloud_point_fwd_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), n, c, X, Wx, Ctr, Y,
                           stats_partial, stat_pivot);
    pcops_note_pipe(0);
    return pcops_launch_status();
}

extern "C" int pcops_cloud_point_bwd(int b, int n, int k, int c, const float *G, const float *Y, const float *p, const float *q,
                                     const float *t, const float *X, const float *Wx, float *dX, float *dWx, float *dCtr,
                                     void *workspace, pcops_stream_t stream) {
    if (!supported(b, n, k, c)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(G); PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(q); PCOPS_REQUIRE_PTR(t);
    PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(Wx); PCOPS_REQUIRE_PTR(dWx); PCOPS_REQUIRE_PTR(dCtr);
    const int splits = bwd_splits(b, n), chunk = bwd_chunk(n, splits);
    const long long parts = (long long)b * splits;
    if (parts > 1) PCOPS_REQUIRE_PTR(workspace);
    hipStream_t hs = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    float *dstW = parts > 1 ? ws : dWx;
    float *wsC = parts > 1 ? ws + parts * kK * c : ws;
    float *dstC = splits > 1 ? wsC : dCtr;
    for (int c0 = 0; c0 < c;) {
        const int left = (c - c0) / kCW;
        const int nch = left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
        static_assert(kPassChunks == 8, "the pass sizes below");
        pcops_dispatch<1, 2, 4, 8>(nch, PCOPS_OK, [&](auto N) {
            launch_bwd_pass<decltype(N)::value>(b, n, c, c0, splits, chunk, G, Y, p, q, t, X, Wx, dX, dstW, dstC, hs);
            return PCOPS_OK;
        });
        c0 += nch * kCW;
    }
    if (parts > 1) {
        const long long len4 = (long long)kK * c / 4;
        hipLaunchKernelGGL(cloud_point_reduce_w_kernel, dim3((unsigned)(len4 / 64)), dim3(kThreads), 0, hs, (int)parts, len4,
                           static_cast<const float *>(ws), dWx);
    }
    if (splits > 1) {
        const long long total = (long long)b * c;
        hipLaunchKernelGGL(cloud_point_reduce_c_kernel, dim3(cdiv(total, kThreads)), dim3(kThreads), 0, hs, splits, c, total,
                           static_cast<const float *>(wsC), dCtr);
    }
    pcops_note_pipe(0);
    return pcops_launch_status();
}
