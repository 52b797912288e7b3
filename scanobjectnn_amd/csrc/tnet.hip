// tnet.hip -- PointNet's learned 64 x 64 feature transform, applied per cloud, and its orthogonality regulariser
// (reference pointnet/models/pointnet_cls.py:47 `tf.matmul(net, transform)` and :86-91) on gfx950.
//
//   forward   out[b][p][:] = X[b][p][:] T[b]                      X, out (b, n, 64), T (b, 64, 64)
//   backward  dX[b] = G[b] T[b]^T,  dT[b] = X[b]^T G[b]           one pass over G
//   ortho     Gm = T T^T - I, loss_parts[b] = w/2 sum Gm^2, dT[b] = 2 w Gm T
//
// Every product runs on v_mfma_f32_16x16x4_f32 with exact fp32 operands.  Lane maps of that instruction (lane l, g = l >> 4,
// l15 = l & 15): A[row = l15][kk = g], B[kk = g][col = l15], C/D row = 4 g + reg, col = l15.  A product sums over kk, so
// WHICH k a lane group feeds in a step is free as long as A and B agree: a lane loads its row of X (or G) as four 16-byte
// pieces, columns 16 jj + 4 g + (0..3), and step (jj, e) multiplies column k = 16 jj + 4 g + e -- coalesced 16-byte loads and
// no shuffle.  The per-cloud matrix is staged once per workgroup in LDS with a row stride of 68 words: a B-operand read is
// M[k][c0 + l15] with k differing by 4 between the two lane groups of a 32-lane half, 4 x 68 = 272 = 16 (mod 32), so the 32
// lanes of a ds_read_b32 group fall on 32 different banks.  The backward stages T transposed (same stride, same reads) and
// the point tile of X and G with a stride of 80 words (rows p and p + 1 of the transposed use X^T G are 16 banks apart).
// Every sum is taken in a fixed order; there is no float atomic in this file.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kK = 64;            // the transform's width
constexpr int kLd = 68;           // LDS row stride of a 64 x 64 matrix
constexpr int kTileLd = 80;       // LDS row stride of the backward's point tile
constexpr int kThreads = 256;     // 4 waves
constexpr int kWaves = kThreads / kWave;
constexpr int kFwdPoints = 128;   // forward: points per workgroup (two 16-point tiles per wave)
constexpr int kPT = 64;           // backward: points per step (one 16-point tile per wave); a split is a whole number of them
constexpr int kSplitCap = 16;     // backward: splits per cloud (a power of two)
constexpr int kTargetWGs = 512;


// M (64, 64) row-major -> LDS [64][68]
__device__ __forceinline__ void stage_plain(const float *__restrict__ M, float *S) {
    for (int e = threadIdx.x; e < kK * kK / 4; e += kThreads) {
        const int i = e >> 4, j = (e & 15) * 4;
        *reinterpret_cast<f32x4 *>(S + i * kLd + j) = reinterpret_cast<const f32x4 *>(M)[e];
    }
}

// M (64, 64) row-major -> its transpose in LDS [64][68]
__device__ __forceinline__ void stage_transposed(const float *__restrict__ M, float *S) {
    for (int e = threadIdx.x; e < kK * kK; e += kThreads) S[(e & 63) * kLd + (e >> 6)] = M[e];
}

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

// acc[t][r] = sum_k row(l15)[k] M[k][16 t + l15] for the 16 rows the wave's lanes hold (D row = 4 g + r); M in LDS, stride 68
__device__ __forceinline__ void rows_times(const f32x4 a[4], const float *M, int g, int l15, f32x4 acc[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *row = M + (16 * jj + 4 * g + e) * kLd + l15;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj][e], row[16 * t], acc[t], 0, 0, 0);
        }
    }
}

// the 16 x 64 tile of rows p0 .. p0 + 15 of a (n, 64) cloud from its D layout
__device__ __forceinline__ void store_rows(float *__restrict__ cloud, int p0, int n, int g, int l15, const f32x4 acc[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = p0 + 4 * g + r;
        if (p >= n) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) cloud[(size_t)p * kK + 16 * t + l15] = acc[t][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (ceil(n / 128), b): all points of a workgroup belong to cloud blockIdx.y
__global__ void __launch_bounds__(kThreads) transformk_fwd_kernel(int n, const float *__restrict__ X,
                                                                  const float *__restrict__ T, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Ts[kK * kLd];
    const size_t cloud = blockIdx.y;
    stage_plain(T + cloud * kK * kK, Ts);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const float *Xc = X + cloud * n * kK;
    float *Oc = out + cloud * n * kK;
    for (int tile = wave; tile < kFwdPoints / 16; tile += kWaves) {
        const int p0 = blockIdx.x * kFwdPoints + tile * 16;
        if (p0 >= n) break;
        f32x4 a[4], acc[4];
        load_row(Xc, p0 + l15, n, g, a);
        rows_times(a, Ts, g, l15, acc);
        store_rows(Oc, p0, n, g, l15, acc);
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// grid (splits, b).  Split s of cloud c takes the points [s chunk, (s + 1) chunk) below n, 64 per step: each wave loads 16
// rows of G and X once, forms its rows of dX = G T^T from the registers, and leaves both tiles in LDS, from which wave w
// accumulates rows 16 w .. 16 w + 15 of X^T G.  dst is dT (one split) or the workspace [b][splits][64][64]; a split that
// holds no point stores zeros.
template <bool DX>
__global__ void __launch_bounds__(kThreads) transformk_bwd_kernel(int n, int chunk, const float *__restrict__ X,
                                                                  const float *__restrict__ T, const float *__restrict__ G,
                                                                  float *__restrict__ dX, float *__restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float Tt[DX ? kK * kLd : 4];
    __shared__ __attribute__((aligned(16))) float Xs[kPT * kTileLd];
    __shared__ __attribute__((aligned(16))) float Gs[kPT * kTileLd];
    const size_t cloud = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const int pbeg = min((long long)blockIdx.x * chunk, (long long)n), pend = min((long long)pbeg + chunk, (long long)n);
    if constexpr (DX) {
        stage_transposed(T + cloud * kK * kK, Tt);
        __syncthreads();
    }
    const float *Xc = X + cloud * n * kK, *Gc = G + cloud * n * kK;
    f32x4 accT[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) accT[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p0 = pbeg; p0 < pend; p0 += kPT) {
        const int pw = p0 + 16 * wave;
        f32x4 xr[4], gr[4];
        load_row(Xc, pw + l15, pend, g, xr);
        load_row(Gc, pw + l15, pend, g, gr);
        float *xs = Xs + (16 * wave + l15) * kTileLd + 4 * g, *gs = Gs + (16 * wave + l15) * kTileLd + 4 * g;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            *reinterpret_cast<f32x4 *>(xs + 16 * jj) = xr[jj];
            *reinterpret_cast<f32x4 *>(gs + 16 * jj) = gr[jj];
        }
        if constexpr (DX) {
            if (pw < pend) {
                f32x4 acc[4];
                rows_times(gr, Tt, g, l15, acc);
                store_rows(dX + cloud * n * kK, pw, pend, g, l15, acc);
            }
        }
        __syncthreads();
        // dT[i = 16 w + l15 as A row][j]: A[row = i][kk = p] = Xs[p][i], B[kk = p][col = j] = Gs[p][j]
#pragma unroll 4
        for (int s = 0; s < kPT / 4; ++s) {
            const int pl = 4 * s + g;
            const float av = Xs[pl * kTileLd + 16 * wave + l15];
            const float *grow = Gs + pl * kTileLd + l15;
#pragma unroll
            for (int t = 0; t < 4; ++t) accT[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, grow[16 * t], accT[t], 0, 0, 0);
        }
        __syncthreads();
    }
    float *o = dst + (cloud * gridDim.x + blockIdx.x) * kK * kK;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) o[(16 * wave + 4 * g + r) * kK + 16 * t + l15] = accT[t][r];
}

// dT[c][e] = ws[c][0][e] + ws[c][1][e] + ... in ascending order; a thread owns four neighbouring elements (len4 = b 64 64 / 4)
// and has SPLITS independent 16-byte loads in flight before the first add
template <int SPLITS>
__global__ void __launch_bounds__(kThreads) transformk_reduce_kernel(long long len4, const float *__restrict__ ws,
                                                                     float *__restrict__ dT) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= len4) return;
    constexpr int kM4 = kK * kK / 4;
    const long long cloud = i / kM4, e = i - cloud * kM4;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(ws) + cloud * SPLITS * kM4 + e;
    f32x4 part[SPLITS];
#pragma unroll
    for (int z = 0; z < SPLITS; ++z) part[z] = src[(size_t)z * kM4];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < SPLITS; ++z) v += part[z];
    reinterpret_cast<f32x4 *>(dT)[i] = v;
}

// ------------------------------------------------------------------------------------------------------------ regulariser
// grid (b).  Gm = T T^T - I from the transposed image alone (A[row = i][kk = j] = Tt[j][i], B[kk = j][col = i'] = Tt[j][i']);
// Gm goes to LDS and, being symmetric bit for bit (both halves add the same products in the same order), is read back as
// A[row = i][kk = i'] = Gm[i'][i] for Gm T against the plain image.
__global__ void __launch_bounds__(kThreads) ortho_reg_kernel(const float *__restrict__ T, float weight,
                                                             float *__restrict__ loss_parts, float *__restrict__ dT) {
    __shared__ __attribute__((aligned(16))) float Ts[kK * kLd];
    __shared__ float Tt[kK * kLd];
    __shared__ float Gm[kK * kLd];
    __shared__ float red[kWaves];
    const size_t cloud = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    stage_plain(T + cloud * kK * kK, Ts);
    stage_transposed(T + cloud * kK * kK, Tt);
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < kK / 4; ++s) {
        const float *row = Tt + (4 * s + g) * kLd + l15;
        const float av = row[16 * wave];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, row[16 * t], acc[t], 0, 0, 0);
    }
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wave + 4 * g + r, i2 = 16 * t + l15;
            const float v = acc[t][r] - (i == i2 ? 1.f : 0.f);
            Gm[i * kLd + i2] = v;
            sq = fmaf(v, v, sq);
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) loss_parts[cloud] = weight * 0.5f * (((red[0] + red[1]) + red[2]) + red[3]);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < kK / 4; ++s) {
        const int i2 = 4 * s + g;
        const float av = Gm[i2 * kLd + 16 * wave + l15];
        const float *row = Ts + i2 * kLd + l15;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, row[16 * t], acc[t], 0, 0, 0);
    }
    const float scale = 2.f * weight;
    float *o = dT + cloud * kK * kK;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) o[(16 * wave + 4 * g + r) * kK + 16 * t + l15] = scale * acc[t][r];
}

bool supported(int b, int n, int k) {
    return k == kK && b >= 1 && b <= 65535 && n >= 1 && (long long)b * n * kK < (1ll << 31);
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

}  // namespace

extern "C" int pcops_transformk_supported(int b, int n, int k) { return supported(b, n, k) ? 1 : 0; }

extern "C" int pcops_transformk_bwd_splits(int b, int n, int k) { return supported(b, n, k) ? bwd_splits(b, n) : 0; }

extern "C" unsigned long long pcops_transformk_workspace_bytes(int b, int n, int k) {
    const int splits = pcops_transformk_bwd_splits(b, n, k);
    if (splits <= 1) return 0;
    return (unsigned long long)b * splits * kK * kK * sizeof(float);
}

extern "C" int pcops_transformk_fwd(int b, int n, int k, const float *X, const float *T, float *out, pcops_stream_t stream) {
    if (!supported(b, n, k)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(T); PCOPS_REQUIRE_PTR(out);
    hipLaunchKernelGGL(transformk_fwd_kernel, dim3(cdiv(n, kFwdPoints), b), dim3(kThreads), 0, as_stream(stream), n, X, T, out);
    pcops_note_pipe(0);
    return pcops_launch_status();
}

extern "C" int pcops_transformk_bwd(int b, int n, int k, const float *X, const float *T, const float *G, float *dX, float *dT,
                                    void *workspace, pcops_stream_t stream) {
    if (!supported(b, n, k)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(T); PCOPS_REQUIRE_PTR(G); PCOPS_REQUIRE_PTR(dT);
    const int splits = bwd_splits(b, n), chunk = bwd_chunk(n, splits);
    if (splits > 1) PCOPS_REQUIRE_PTR(workspace);
    hipStream_t hs = as_stream(stream);
    float *dst = splits > 1 ? static_cast<float *>(workspace) : dT;
    if (dX)
        hipLaunchKernelGGL(transformk_bwd_kernel<true>, dim3(splits, b), dim3(kThreads), 0, hs, n, chunk, X, T, G, dX, dst);
    else
        hipLaunchKernelGGL(transformk_bwd_kernel<false>, dim3(splits, b), dim3(kThreads), 0, hs, n, chunk, X, T, G, dX, dst);
    if (splits > 1) {
        const long long len4 = (long long)b * kK * kK / 4;
        pcops_dispatch<2, 4, 8, 16>(splits, PCOPS_OK, [&](auto S) {
            hipLaunchKernelGGL(transformk_reduce_kernel<decltype(S)::value>, dim3(cdiv(len4, kThreads)), dim3(kThreads), 0, hs,
                               len4, static_cast<const float *>(workspace), dT);
            return PCOPS_OK;
        });
    }
    pcops_note_pipe(0);
    return pcops_launch_status();
}

extern "C" int pcops_ortho_reg(int b, int k, const float *T, float weight, float *loss_parts, float *dT,
                               pcops_stream_t stream) {
    if (k != kK || b < 1 || b > 65535) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(T); PCOPS_REQUIRE_PTR(loss_parts); PCOPS_REQUIRE_PTR(dT);
    hipLaunchKernelGGL(ortho_reg_kernel, dim3(b), dim3(kThreads), 0, as_stream(stream), T, weight, loss_parts, dT);
    pcops_note_pipe(0);
    return pcops_launch_status();
}
