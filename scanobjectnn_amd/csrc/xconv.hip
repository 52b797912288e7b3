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
//
// Channel groups (WIDE).  A wave walks its point's channel tiles one after the other, each a dependent chain (load, 4 MFMA,
// shuffle, store), and the launch has one wave per point: a layer of 36 tiles on 4096 points is a long chain on about one
// wave per SIMD.  The tiles are independent, so with more than kOneGroupTiles of them the forward and the data gradient put
// them on the grid's y axis: group y owns the tiles [y t, (y + 1) t), t <= kGroupTiles, stages only its own columns of wd
// (row stride t 16 dm, zero past its last channel) and runs the same arithmetic per element -- out, dlifted and dfts_grouped
// keep the one-group bits.  dX is a sum over the tiles: group y stores its partial to slice y of a workspace and
// xconv_reduce_kernel adds the slices in ascending order.  WIDE = false is the one-group kernel as it was.
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
constexpr int kOneGroupTiles = 16;  // forward / dgrad: up to this many channel tiles (c <= 256) one group walks them all
constexpr int kGroupTiles = 8;      // ... beyond it ceil(tiles / 8) groups of at most 8 tiles


struct Shape {
    int n, p, K, c1, c2, c, cd;   // points per cloud, representatives per cloud, neighbours, channels, c dm
};

// wd (K, c, dm) -> LDS [16][c dm], rows K..15 zero
__device__ __forceinline__ void stage_wd(const Shape &s, const float *__restrict__ wd, float *wds) {
    const int len = kKP * s.cd, have = s.K * s.cd;
    for (int e = threadIdx.x; e < len; e += kThreads) wds[e] = e < have ? wd[e] : 0.f;
    __syncthreads();
}

// the channels [lo, hi) a workgroup owns and the row stride of its wd image in LDS
struct Slice {
    int lo, hi, ld;
};

// WIDE: group blockIdx.y of tpg tiles each; its image is wd[:, lo:hi, :] -> LDS [16][tpg 16 dm], zero past K rows and past hi.
// Otherwise all of it, staged as above.
template <int DM, bool WIDE>
__device__ __forceinline__ Slice stage_slice(const Shape &s, int tpg, const float *__restrict__ wd, float *wds) {
    if constexpr (!WIDE) {
        stage_wd(s, wd, wds);
        return Slice{0, s.c, s.cd};
    } else {
        const int lo = min((int)blockIdx.y * tpg * kCT, s.c), hi = min(lo + tpg * kCT, s.c);
        const int ld = tpg * kCT * DM, have = (hi - lo) * DM;
        for (int e = threadIdx.x; e < kKP * ld; e += kThreads) {
            const int row = e / ld, col = e - row * ld;
            wds[e] = (row < s.K && col < have) ? wd[(size_t)row * s.cd + lo * DM + col] : 0.f;
        }
        __syncthreads();
        return Slice{lo, hi, ld};
    }
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
__device__ __forceinline__ f32x4 xfin_tile(const Shape &s, long long q, int c0, int g, int l15, const float *xa,
                                        const float *__restrict__ lifted, const float *__restrict__ fts,
                                        const int *__restrict__ idx) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float bv = load_fin(s, q, 4 * j + g, c0 + l15, lifted, fts, idx);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j], bv, acc, 0, 0, 0);
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (ceil(P / 16), groups); tpg: tiles per group (read by WIDE only)
template <int DM, bool WIDE>
__global__ void __launch_bounds__(kThreads) xconv_fwd_kernel(Shape s, long long P, int tpg, const float *__restrict__ lifted,
                                                             const float *__restrict__ fts, const int *__restrict__ idx,
                                                             const float *__restrict__ X, const float *__restrict__ wd,
                                                             float *__restrict__ out) {
    extern __shared__ float wds[];
    const Slice sl = stage_slice<DM, WIDE>(s, tpg, wd, wds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const long long q0 = (long long)blockIdx.x * kPointsPerWG;
    const long long qend = q0 + kPointsPerWG < P ? q0 + kPointsPerWG : P;
    for (long long q = q0 + wave; q < qend; q += kWaves) {
        float xa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[j] = load_x(s, q, l15, 4 * j + g, X);
        for (int c0 = sl.lo; c0 < sl.hi; c0 += kCT) {
            const f32x4 t = xfin_tile(s, q, c0, g, l15, xa, lifted, fts, idx);
            const int ch = c0 + l15;
            const bool ok = ch < sl.hi;
#pragma unroll
            for (int m = 0; m < DM; ++m) {
                float v = 0.f;
                if (ok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v = fmaf(wds[(4 * g + r) * sl.ld + (ch - sl.lo) * DM + m], t[r], v);
                }
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (ok && g == 0) out[(size_t)q * s.cd + ch * DM + m] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- data gradient
// dT[kp][ch] = sum_m wd[kp,ch,m] dout[q, ch dm + m]; zero past the slice (rows past K are zero in wds)
template <int DM>
__device__ __forceinline__ float dt_at(const Slice &sl, const float *wds, const float *__restrict__ dyq, int kp, int ch) {
    if (ch >= sl.hi) return 0.f;
    float v = 0.f;
#pragma unroll
    for (int m = 0; m < DM; ++m) v = fmaf(wds[kp * sl.ld + (ch - sl.lo) * DM + m], dyq[ch * DM + m], v);
    return v;
}

// grid (ceil(P / 16), groups).  WIDE: dX is the workspace [groups][P][K][K], group blockIdx.y stores its partial sum to
// its own slice; dlifted and dfg are per channel and go straight out.
template <int DM, bool WIDE>
__global__ void __launch_bounds__(kThreads) xconv_dgrad_kernel(Shape s, long long P, int tpg, const float *__restrict__ lifted,
                                                               const float *__restrict__ fts, const int *__restrict__ idx,
                                                               const float *__restrict__ X, const float *__restrict__ wd,
                                                               const float *__restrict__ dy, float *__restrict__ dX,
                                                               float *__restrict__ dlifted, float *__restrict__ dfg) {
    extern __shared__ float wds[];
    const Slice sl = stage_slice<DM, WIDE>(s, tpg, wd, wds);
    if constexpr (WIDE) dX += (size_t)blockIdx.y * P * s.K * s.K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
    const long long q0 = (long long)blockIdx.x * kPointsPerWG;
    const long long qend = q0 + kPointsPerWG < P ? q0 + kPointsPerWG : P;
    for (long long q = q0 + wave; q < qend; q += kWaves) {
        const float *dyq = dy + (size_t)q * s.cd;
        float xt[4];                                   // A[row = k = l15][kk = g] of step j: X[k' = 4 j + g][k = l15]
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = load_x(s, q, 4 * j + g, l15, X);
        f32x4 accX = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = sl.lo; c0 < sl.hi; c0 += kCT) {
            // dFin[k = 4 g + reg][ch = c0 + l15] = sum_k' X[k',k] dT[k',ch]
            f32x4 accF = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                accF = __builtin_amdgcn_mfma_f32_16x16x4f32(xt[j], dt_at<DM>(sl, wds, dyq, 4 * j + g, c0 + l15), accF, 0,
                                                            0, 0);
            const int ch = c0 + l15;
            if (ch < sl.hi) {
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
                accX = __builtin_amdgcn_mfma_f32_16x16x4f32(dt_at<DM>(sl, wds, dyq, l15, chA),
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
// ws[z][K][c][dm] (a split without points stores zeros) and xconv_reduce_kernel adds the splits in ascending order.
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
        const f32x4 t = xfin_tile(s, q, c0, g, l15, xa, lifted, fts, idx);
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

// out[i] = ws[0][i] + ws[1][i] + ... in ascending order: the weight gradient's row splits and the data gradient's channel
// groups of dX
__global__ void xconv_reduce_kernel(int len, int splits, const float *__restrict__ ws, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
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

// forward / dgrad: one group up to 16 channel tiles (c <= 256), else ceil(tiles / 8); no group is empty and none holds more
// than 8 tiles for any tile count (tests/test_xdconv_ref_cpu.py walks 1..60)
int channel_groups(int c) {
    const int tiles = cdiv(c, kCT);
    if (tiles <= kOneGroupTiles || pcops_get_option(PCOPS_OPT_XCONV_CHANNEL_GROUPS) == 0) return 1;
    return cdiv(tiles, kGroupTiles);
}

int group_tiles(int c, int groups) { return cdiv(cdiv(c, kCT), groups); }

// the data gradient in `groups` channel groups; workspace [groups][P][K][K] with more than one
int launch_dgrad(const Shape &s, long long P, int dm, int groups, const float *lifted, const float *fts, const int *idx,
                 const float *X, const float *wd, const float *dout, float *dX, float *dlifted, float *dfg, float *ws,
                 hipStream_t hs) {
    return pcops_dispatch<1, 2, 3, 4>(dm, PCOPS_ERR_UNSUPPORTED, [&](auto DM) {
        constexpr int kDM = decltype(DM)::value;
        if (groups == 1) {
            hipLaunchKernelGGL((xconv_dgrad_kernel<kDM, false>), dim3(cdiv(P, kPointsPerWG)), dim3(kThreads),
                               (size_t)kKP * s.cd * sizeof(float), hs, s, P, 0, lifted, fts, idx, X, wd, dout, dX, dlifted,
                               dfg);
        } else {
            const int tpg = group_tiles(s.c, groups), len = (int)(P * s.K * s.K);
            hipLaunchKernelGGL((xconv_dgrad_kernel<kDM, true>), dim3(cdiv(P, kPointsPerWG), groups), dim3(kThreads),
                               (size_t)kKP * tpg * kCT * kDM * sizeof(float), hs, s, P, tpg, lifted, fts, idx, X, wd, dout,
                               ws, dlifted, dfg);
            hipLaunchKernelGGL(xconv_reduce_kernel, dim3(cdiv(len, kThreads)), dim3(kThreads), 0, hs, len, groups, ws, dX);
        }
        pcops_note_pipe(0);
        return pcops_launch_status();
    });
}

}  // namespace

extern "C" int pcops_xconv_supported(int k, int c1, int c2, int dm) { return supported(k, c1, c2, dm) ? 1 : 0; }

extern "C" int pcops_xconv_channel_groups(int b, int n, int p, int k, int c1, int c2, int dm) {
    if (check(b, n, p, k, c1, c2, dm) != PCOPS_OK || b == 0) return 0;
    return channel_groups(c1 + c2);
}

extern "C" unsigned long long pcops_xconv_dgrad_workspace_bytes(int b, int n, int p, int k, int c1, int c2, int dm) {
    const int groups = pcops_xconv_channel_groups(b, n, p, k, c1, c2, dm);
    if (groups <= 1) return 0;
    return (unsigned long long)groups * b * p * k * k * sizeof(float);
}

extern "C" int pcops_xconv_fwd(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted, const float *fts,
                               const int *idx, const float *X, const float *wd, float *out, pcops_stream_t stream) {
    const int st = check(b, n, p, k, c1, c2, dm);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(lifted); PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(wd); PCOPS_REQUIRE_PTR(out);
    if (c2 > 0) { PCOPS_REQUIRE_PTR(fts); PCOPS_REQUIRE_PTR(idx); }
    const Shape s = make_shape(n, p, k, c1, c2, dm);
    const long long P = (long long)b * p;
    const int groups = channel_groups(s.c);
    return pcops_dispatch<1, 2, 3, 4>(dm, PCOPS_ERR_UNSUPPORTED, [&](auto DM) {
        constexpr int kDM = decltype(DM)::value;
        if (groups == 1) {
            hipLaunchKernelGGL((xconv_fwd_kernel<kDM, false>), dim3(cdiv(P, kPointsPerWG)), dim3(kThreads),
                               (size_t)kKP * s.cd * sizeof(float), as_stream(stream), s, P, 0, lifted, fts, idx, X, wd, out);
        } else {
            const int tpg = group_tiles(s.c, groups);
            hipLaunchKernelGGL((xconv_fwd_kernel<kDM, true>), dim3(cdiv(P, kPointsPerWG), groups), dim3(kThreads),
                               (size_t)kKP * tpg * kCT * kDM * sizeof(float), as_stream(stream), s, P, tpg, lifted, fts, idx,
                               X, wd, out);
        }
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
    return launch_dgrad(make_shape(n, p, k, c1, c2, dm), (long long)b * p, dm, 1, lifted, fts, idx, X, wd, dout, dX, dlifted,
                        dfts_grouped, nullptr, as_stream(stream));
}

extern "C" int pcops_xconv_dgrad_ws(int b, int n, int p, int k, int c1, int c2, int dm, const float *lifted,
                                    const float *fts, const int *idx, const float *X, const float *wd, const float *dout,
                                    float *dX, float *dlifted, float *dfts_grouped, void *workspace, pcops_stream_t stream) {
    const int st = check(b, n, p, k, c1, c2, dm);
    if (st != PCOPS_OK) return st;
    if (b == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(lifted); PCOPS_REQUIRE_PTR(X); PCOPS_REQUIRE_PTR(wd); PCOPS_REQUIRE_PTR(dout);
    PCOPS_REQUIRE_PTR(dX); PCOPS_REQUIRE_PTR(dlifted);
    if (c2 > 0) { PCOPS_REQUIRE_PTR(fts); PCOPS_REQUIRE_PTR(idx); }
    const int groups = channel_groups(c1 + c2);
    if (groups > 1) PCOPS_REQUIRE_PTR(workspace);
    return launch_dgrad(make_shape(n, p, k, c1, c2, dm), (long long)b * p, dm, groups, lifted, fts, idx, X, wd, dout, dX,
                        dlifted, dfts_grouped, static_cast<float *>(workspace), as_stream(stream));
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
        (void)pcops_zero_async(dwd, (size_t)len * sizeof(float), hs);
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
            hipLaunchKernelGGL(xconv_reduce_kernel, dim3(cdiv(len, kThreads)), dim3(kThreads), 0, hs, len, splits, ws,
                               dwd);
        pcops_note_pipe(0);
        return pcops_launch_status();
    });
}
