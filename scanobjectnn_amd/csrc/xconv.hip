// xconv.hip -- the X-Conv contraction of PointCNN (reference PointCNN/pointcnn.py:28-44: gather_nd, concat, matmul with
// the X-transform, and the depthwise half of separable_conv2d with a (1, K) kernel) on gfx950.
//
// Per representative point q (P = b p of them), K <= 16 neighbours, c = c1 + c2 channels, dm = depth multiplier:
//   Fin[q,k,:]        = concat(lifted[q,k,:c1], fts[cloud(q), idx[q,k], :c2])
//   T[q,k',ch]        = sum_k X[q,k',k] Fin[q,k,ch]                                  (fts_X of the reference)
//   out[q, ch dm + m] = sum_k' wd[k',ch,m] T[q,k',ch]                                (TF's depthwise channel order)
// Neither Fin nor T is ever written to memory.  One WAVE owns one point: K is zero-padded to 16, so T for 16 channels is
// ONE 16 x 16 accumulator tile of v_mfma_f32_16x16x4_f32, four issues deep (k = 0..15).  Lane maps of that instruction:
// A[l & 15][kk = l >> 4], B[kk = l >> 4][l & 15], C/D col = l & 15, row = 4 (l >> 4) + reg.  With A = X and B = Fin a lane
// ends up with T[k' = 4 g + reg][ch = c0 + (l & 15)], g = l >> 4: the depthwise sum over k' is a four-term fmaf chain in
// the lane and two cross-lane adds (xor 16, xor 32) over the four row groups -- channels never mix, so channel tiles need
// no reduction between them.  The operands are loaded straight into their lanes (X once per point, reused by every
// channel tile); wd, the only operand shared by all points, is staged once per workgroup in LDS, rows K..15 zero.
//
// Backward.  dT[k',ch] = sum_m wd[k',ch,m] dout[ch dm + m] is dm multiply-adds, so each lane forms it directly in whichever
// operand layout the next product wants (no transpose through LDS):
//   dFin[k,ch] = sum_k' X[k',k] dT[k',ch]     A = X^T, B = dT         -> dlifted / dfts_grouped, written from the D tile
//   dX[k',k]   = sum_ch dT[k',ch] Fin[k,ch]   A = dT,  B = Fin^T      -> accumulated over the channel tiles
//   dwd[k',ch,m] = sum_q T[q,k',ch] dout[q, ch dm + m]: T recomputed by the forward's MFMA; the lane that holds
//   T[k',ch] keeps the sum over its points in registers.  Row splits -> workspace -> one fixed-order pass.
// Every sum is taken in a fixed order; there is no float atomic in this file.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kKP = 16;          // K padded to the MFMA tile
constexpr int kCT = 16;          // channels per tile
constexpr int kThreads = 256;    // 4 waves
constexpr int kWaves = kThreads / kWave;
constexpr int kPointsPerWG = 16; // forward / dgrad: points per workgroup (4 per wave), amortises the wd staging
constexpr int kMaxCD = 960;      // c dm: 16 rows of it are 61 440 bytes of LDS
constexpr int kSplitCap = 64;    // weight gradient: row splits (a power of two)
constexpr int kSplitRows = 16;   // ... each a whole number of 16-point steps
constexpr int kTargetWGs = 512;

typedef float f4 __attribute__((ext_vector_type(4)));

struct Shape {
    int n, p, K, c1, c2, c, cd;   // points per cloud, representatives per cloud, neighbours, channels, c dm
};

// wd (K, c, dm) -> LDS [16][c dm], rows K..15 zero
__device__ __forceinline__ void stage_wd(const Shape &s, const float *__restrict__ wd, float *wds) {
    const int len = kKP * s.cd, have = s.K * s.cd;
    for (int e = threadIdx.x; e < len; e += kThreads) wds[e] = e < have ? wd[e] : 0.f;
    __syncthreads();
}

// Fin[q, k, ch], zero outside K x c
__device__ __forceinline__ float load_fin(const Shape &s, long long q, int k, int ch, const float *__restrict__ lifted,
                                          const float *__restrict__ fts, const int *__restrict__ idx) {
    if (k >= s.K || ch >= s.c) return 0.f;
    if (ch < s.c1) return lifted[((size_t)q * s.K + k) * s.c1 + ch];
    const size_t row = (size_t)(q / s.p) * s.n + idx[(size_t)q * s.K + k];
    return fts[row * s.c2 + (ch - s.c1)];
}

// X[q, k', k], zero outside K x K
__device__ __forceinline__ float load_x(const Shape &s, long long q, int kp, int k, const float *__restrict__ X) {
    return (kp < s.K && k < s.K) ? X[((size_t)q * s.K + kp) * s.K + k] : 0.f;
}

// T[k' = 4 g + reg][ch = c0 + l15] of point q; xa[j] = X[k' = l15][k = 4 j + g]
__device__ __forceinline__ f4 xfin_tile(const Shape &s, long long q, int c0, int g, int l15, const float *xa,
                                        const float *__restrict__ lifted, const float *__restrict__ fts,
                                        const int *__restrict__ idx) {
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float bv = load_fin(s, q, 4 * j + g, c0 + l15, lifted, fts, idx);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j], bv, acc, 0, 0, 0);
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int DM>
__global__ void __launch_bounds__(kThreads) xconv_fwd_kernel(Shape s, long long P, const float *__restrict__ lifted,
                                                             const float *__restrict__ fts, const int *__restrict__ idx,
                                                             const float *__restrict__ X, const float *__restrict__ wd,
                                                             float *__restrict__ out) {
    extern __shared__ float wds[];
    stage_wd(s, wd, wds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const long long q0 = (long long)blockIdx.x * kPointsPerWG;
    const long long qend = q0 + kPointsPerWG < P ? q0 + kPointsPerWG : P;
    for (long long q = q0 + wave; q < qend; q += kWaves) {
        float xa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[j] = load_x(s, q, l15, 4 * j + g, X);
        for (int c0 = 0; c0 < s.c; c0 += kCT) {
            const f4 t = xfin_tile(s, q, c0, g, l15, xa, lifted, fts, idx);
            const int ch = c0 + l15;
            const bool ok = ch < s.c;
#pragma unroll
            for (int m = 0; m < DM; ++m) {
                float v = 0.f;
                if (ok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v = fmaf(wds[(4 * g + r) * s.cd + ch * DM + m], t[r], v);
                }
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (ok && g == 0) out[(size_t)q * s.cd + ch * DM + m] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- data gradient
// dT[kp][ch] = sum_m wd[kp,ch,m] dout[q, ch dm + m]; zero past c (rows past K are zero in wds)
template <int DM>
__device__ __forceinline__ float dt_at(const Shape &s, const float *wds, const float *__restrict__ dyq, int kp, int ch) {
    if (ch >= s.c) return 0.f;
    float v = 0.f;
#pragma unroll
    for (int m = 0; m < DM; ++m) v = fmaf(wds[kp * s.cd + ch * DM + m], dyq[ch * DM + m], v);
    return v;
}

template <int DM>
__global__ void __launch_bounds__(kThreads) xconv_dgrad_kernel(Shape s, long long P, const float *__restrict__ lifted,
                                                               const float *__restrict__ fts, const int *__restrict__ idx,
                                                               const float *__restrict__ X, const float *__restrict__ wd,
                                                               const float *__restrict__ dy, float *__restrict__ dX,
                                                               float *__restrict__ dlifted, float *__restrict__ dfg) {
    extern __shared__ float wds[];
    stage_wd(s, wd, wds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const long long q0 = (long long)blockIdx.x * kPointsPerWG;
    const long long qend = q0 + kPointsPerWG < P ? q0 + kPointsPerWG : P;
    for (long long q = q0 + wave; q < qend; q += kWaves) {
        const float *dyq = dy + (size_t)q * s.cd;
        float xt[4];                                   // A[row = k = l15][kk = g] of step j: X[k' = 4 j + g][k = l15]
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = load_x(s, q, 4 * j + g, l15, X);
        f4 accX = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < s.c; c0 += kCT) {
            // dFin[k = 4 g + reg][ch = c0 + l15] = sum_k' X[k',k] dT[k',ch]
            f4 accF = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                accF = __builtin_amdgcn_mfma_f32_16x16x4f32(xt[j], dt_at<DM>(s, wds, dyq, 4 * j + g, c0 + l15), accF, 0,
                                                            0, 0);
            const int ch = c0 + l15;
            if (ch < s.c) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 4 * g + r;
                    if (k >= s.K) continue;
                    if (ch < s.c1) dlifted[((size_t)q * s.K + k) * s.c1 + ch] = accF[r];
                    else if (dfg) dfg[((size_t)q * s.K + k) * s.c2 + (ch - s.c1)] = accF[r];
                }
            }
            // dX[k' = 4 g + reg][k = l15] += sum over this tile's channels of dT[k',ch] Fin[k,ch]
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int chA = c0 + 4 * j + g;
                accX = __builtin_amdgcn_mfma_f32_16x16x4f32(dt_at<DM>(s, wds, dyq, l15, chA),
                                                            load_fin(s, q, l15, chA, lifted, fts, idx), accX, 0, 0, 0);
            }
        }
        if (l15 < s.K) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g + r < s.K) dX[((size_t)q * s.K + 4 * g + r) * s.K + l15] = accX[r];
        }
    }
}

// -------------------------------------------------------------------------------------------------------- weight gradient
// grid (ceil(c / 16), splits).  Split z takes the points [z chunk, (z + 1) chunk), its four waves every fourth of them in
// ascending order; the waves' sums are added in wave order through LDS.  With splits > 1 the result goes to
// ws[z][K][c][dm] (a split without points stores zeros) and xconv_wgrad_reduce_kernel adds the splits in ascending order.
template <int DM>
__global__ void __launch_bounds__(kThreads) xconv_wgrad_kernel(Shape s, long long P, long long chunk,
                                                               const float *__restrict__ lifted,
                                                               const float *__restrict__ fts, const int *__restrict__ idx,
                                                               const float *__restrict__ X, const float *__restrict__ dy,
                                                               float *__restrict__ dst) {
    __shared__ float red[kWaves][4 * DM][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const int c0 = blockIdx.x * kCT, ch = c0 + l15;
    const long long pbeg = (long long)blockIdx.y * chunk;
    const long long pend = pbeg + chunk < P ? pbeg + chunk : P;
    float acc[4][DM];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < DM; ++m) acc[r][m] = 0.f;
    for (long long q = pbeg + wave; q < pend; q += kWaves) {
        float xa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[j] = load_x(s, q, l15, 4 * j + g, X);
        const f4 t = xfin_tile(s, q, c0, g, l15, xa, lifted, fts, idx);
        if (ch < s.c) {
#pragma unroll
            for (int m = 0; m < DM; ++m) {
                const float d = dy[(size_t)q * s.cd + ch * DM + m];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r][m] = fmaf(t[r], d, acc[r][m]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < DM; ++m) red[wave][r * DM + m][lane] = acc[r][m];
    __syncthreads();
    if (wave != 0 || ch >= s.c) return;
    float *o = dst + (size_t)blockIdx.y * s.K * s.cd;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kp = 4 * g + r;
        if (kp >= s.K) continue;
#pragma unroll
        for (int m = 0; m < DM; ++m) {
            float v = red[0][r * DM + m][lane];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += red[w][r * DM + m][lane];
            o[(size_t)kp * s.cd + ch * DM + m] = v;
        }
    }
}

__global__ void xconv_wgrad_reduce_kernel(int len, int splits, const float *__restrict__ ws, float *__restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= len) return;
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += ws[(size_t)z * len + i];
    out[i] = v;
}

bool supported(int k, int c1, int c2, int dm) {
    return k >= 1 && k <= kKP && c1 >= 1 && c2 >= 0 && dm >= 1 && dm <= 4 && (long long)(c1 + c2) * dm <= kMaxCD;
}

// PCOPS_OK, or why the launchers refuse the shape (before any pointer is looked at)
int check(int b, int n, int p, int k, int c1, int c2, int dm) {
    PCOPS_REQUIRE_SHAPE(b >= 0 && n > 0 && p > 0 && k > 0 && c1 > 0 && c2 >= 0 && dm > 0);
    if (!supported(k, c1, c2, dm)) return PCOPS_ERR_UNSUPPORTED;
    const long long P = (long long)b * p, widest = std::max((c1 + c2) * dm, k);
    if (P * k * widest >= (1ll << 31) || (long long)b * n * std::max(c2, 1) >= (1ll << 31)) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}

Shape make_shape(int n, int p, int k, int c1, int c2, int dm) {
    return Shape{n, p, k, c1, c2, c1 + c2, (c1 + c2) * dm};
}

// the largest power of two that keeps >= 16 points per split and stops once the grid has kTargetWGs workgroups
int wgrad_splits(int b, int p, int c) {
    const long long P = (long long)b * p, tiles = (c + kCT - 1) / kCT;
    long long want = std::min<long long>((kTargetWGs + tiles - 1) / tiles, P / kSplitRows);
    want = std::min<long long>(want, kSplitCap);
    int s = 1;
    while (2 * s <= want) s *= 2;
    return s;
}

long long wgrad_chunk(long long P, int splits) {
    const long long per = (P + splits - 1) / splits;
    return (per + kSplitRows - 1) / kSplitRows * kSplitRows;
}

}  // namespace

extern "C" int pcops_xconv_supported(int k, int c1, int c2, int dm) { return supported(k, c1, c2, dm) ? 1 : 0; }

extern "C" int pcops_xconv_fwd(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                               const int *idx, const float *X, const float *wd, float *out, pcops_stream_t stream) {
    const int st = check(b, n, p, k, c1, c2, dm);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(lifted); PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(wd); PCOPS_REQUIRE_PTR(out);
    if (c2 > 0) { PCOPS_REQUIRE_PTR(fts); PCOPS_REQUIRE_PTR(idx); }
    const Shape s = make_shape(n, p, k, c1, c2, dm);
    const long long P = (long long)b * p;
    const size_t lds = (size_t)kKP * s.cd * sizeof(float);
    return pcops_dispatch<1, 2, 3, 4>(dm, PCOPS_ERR_UNSUPPORTED, [&](auto DM) {
        hipLaunchKernelGGL(xconv_fwd_kernel<decltype(DM)::value>, dim3(cdiv(P, kPointsPerWG)), dim3(kThreads), lds,
                           as_stream(stream), s, P, lifted, fts, idx, X, wd, out);
        pcops_note_pipe(0);
        return pcops_launch_status();
    });
}

extern "C" int pcops_xconv_dgrad(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                                 const int *idx, const float *X, const float *wd, const float *dout, float *dX,
                                 float *dlifted, float *dfts_grouped, pcops_stream_t stream) {
    const int st = check(b, n, p, k, c1, c2, dm);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(lifted); PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(wd); PCOPS_REQUIRE_PTR(dout);
    PCOPS_REQUIRE_PTR(dX); PCOPS_REQUIRE_PTR(dlifted);
    if (c2 > 0) { PCOPS_REQUIRE_PTR(fts); PCOPS_REQUIRE_PTR(idx); }
    const Shape s = make_shape(n, p, k, c1, c2, dm);
    const long long P = (long long)b * p;
    const size_t lds = (size_t)kKP * s.cd * sizeof(float);
    return pcops_dispatch<1, 2, 3, 4>(dm, PCOPS_ERR_UNSUPPORTED, [&](auto DM) {
        hipLaunchKernelGGL(xconv_dgrad_kernel<decltype(DM)::value>, dim3(cdiv(P, kPointsPerWG)), dim3(kThreads), lds,
                           as_stream(stream), s, P, lifted, fts, idx, X, wd, dout, dX, dlifted, dfts_grouped);
        pcops_note_pipe(0);
        return pcops_launch_status();
    });
}

extern "C" int pcops_xconv_wgrad_splits(int b, int n, int p, int k, int c1, int c2, int dm) {
    if (check(b, n, p, k, c1, c2, dm) != PCOPS_OK || b == 0) return 0;
    return wgrad_splits(b, p, c1 + c2);
}

extern "C" unsigned long long pcops_xconv_wgrad_workspace_bytes(int b, int n, int p, int k, int c1, int c2, int dm) {
    const int splits = pcops_xconv_wgrad_splits(b, n, p, k, c1, c2, dm);
    if (splits <= 1) return 0;
    return (unsigned long long)splits * k * (c1 + c2) * dm * sizeof(float);
}

extern "C" int pcops_xconv_wgrad(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                                 const int *idx, const float *X, const float *dout, float *dwd, void *workspace,
                                 pcops_stream_t stream) {
    const int st = check(b, n, p, k, c1, c2, dm);
    if (st != PCOPS_OK) return st;
    PCOPS_REQUIRE_PTR(dwd);
    hipStream_t hs = as_stream(stream);
    const Shape s = make_shape(n, p, k, c1, c2, dm);
    const int len = k * s.cd;
    if (b == 0) {
        (void)hipMemsetAsync(dwd, 0, (size_t)len * sizeof(float), hs);
        return pcops_launch_status();
    }
    PCOPS_REQUIRE_PTR(lifted); PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(dout);
    if (c2 > 0) { PCOPS_REQUIRE_PTR(fts); PCOPS_REQUIRE_PTR(idx); }
    const int splits = wgrad_splits(b, p, s.c);
    if (splits > 1) PCOPS_REQUIRE_PTR(workspace);
    const long long P = (long long)b * p, chunk = wgrad_chunk(P, splits);
    float *ws = static_cast<float *>(workspace);
    return pcops_dispatch<1, 2, 3, 4>(dm, PCOPS_ERR_UNSUPPORTED, [&](auto DM) {
        hipLaunchKernelGGL(xconv_wgrad_kernel<decltype(DM)::value>, dim3(cdiv(s.c, kCT), splits), dim3(kThreads), 0, hs, s,
                           P, chunk, lifted, fts, idx, X, dout, splits > 1 ? ws : dwd);
        if (splits > 1)
            hipLaunchKernelGGL(xconv_wgrad_reduce_kernel, dim3(cdiv(len, kThreads)), dim3(kThreads), 0, hs, len, splits, ws,
                               dwd);
        pcops_note_pipe(0);
        return pcops_launch_status();
    });
}
