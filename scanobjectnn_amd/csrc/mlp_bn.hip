// mlp_bn.hip -- the per-channel and elementwise passes around the matrix products of mlp.hip (same contract: the shared
// per-point MLP of pcops.h, 1x1 conv + bias + BatchNorm + ReLU [+ max-pool over the neighbourhood]):
//
//   statistics    the products' epilogues leave partial rows [P][2][N] of per-channel sums; colreduce_stage1 + bn_finalize /
//                 bn_bwd_coeffs turn them into (mean, rstd, scale, shift) and (dgamma, dbeta, p, q, t); P <= kFusedRows rows
//                 take one launch (the *_fused kernels).  Sums in double, in a fixed order.
//   pooling       BN + ReLU + max over a neighbourhood with the arg-max (whole groups and compacted rows), the pick among a
//                 group's per-block partials, the pooled gradient's mask and statistics
//   elementwise   BN + ReLU of a tensor, the ReLU mask with the two BN-backward sums
//   partial sums  sum_partials2_kernel closes every product kernel that writes a partial copy per workgroup; mlp.hip's build
//                 parts and pooltop_sparse.hip reach it through pcops_mlp_sum_partials2 (declared in common.h)
//   transpose     Wt = W^T of a weight matrix
// The kernels keep the names they had in mlp.hip (pcops_mlp::(anonymous namespace)::...): the profiles know them by those.
#include "common.h"

namespace pcops_mlp {
namespace {

// ---------------------------------------------------------------------------------------------
// column reduction of partial statistics [P][2][N] -> double [2][N], two stages, deterministic
constexpr int kRedSlices = 32;

__global__ __launch_bounds__(256) void colreduce_stage1(int P, int N, const float *__restrict__ part,
                                                        double *__restrict__ ws) {
    // grid (ceil(N/32), 2, kRedSlices); thread (c = tid%32, g = tid/32)
    __shared__ double sm[8][32];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), g = threadIdx.x >> 5;
    const int which = blockIdx.y, slice = blockIdx.z;
    const int per = (P + kRedSlices - 1) / kRedSlices;
    const int p0 = slice * per, p1 = min(P, p0 + per);
    double s = 0.0;
    if (c < N)
        for (int p = p0 + g; p < p1; p += 8) s += (double)part[((long long)p * 2 + which) * N + c];
    sm[g][threadIdx.x & 31] = s;
    __syncthreads();
    if (g == 0 && c < N) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) t += sm[i][threadIdx.x];
        ws[((long long)slice * 2 + which) * N + c] = t;
    }
}

// forward BN: statistics -> (mean, rstd, scale, shift) and the moving-average update
__global__ __launch_bounds__(256) void bn_finalize_kernel(int N, double R, const double *__restrict__ ws,
                                                          const float *__restrict__ pivot,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float eps,
                                                          float decay, int unbiased,
                                                          float *__restrict__ moving_mean,
                                                          float *__restrict__ moving_var,
                                                          float *__restrict__ mean_o, float *__restrict__ rstd_o,
                                                          float *__restrict__ scale_o, float *__restrict__ shift_o) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < kRedSlices; ++s) {
        s1 += ws[((long long)s * 2 + 0) * N + c];
        s2 += ws[((long long)s * 2 + 1) * N + c];
    }
    // the sums are those of (y - pivot) and (y - pivot)^2: the shift leaves the variance untouched and is added back
    // to the mean; with the pivot near the mean the subtraction below no longer cancels leading digits
    const double dm = s1 / R;
    const double mean = dm + (pivot ? (double)pivot[c] : 0.0);
    double var = s2 / R - dm * dm;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * rstd;
    mean_o[c] = (float)mean;
    rstd_o[c] = rstd;
    scale_o[c] = sc;
    shift_o[c] = beta[c] - (float)mean * sc;
    if (moving_mean) {
        const double uv = (unbiased && R > 1.0) ? var * (R / (R - 1.0)) : var;
        moving_mean[c] = decay * moving_mean[c] + (1.f - decay) * (float)mean;
        moving_var[c] = decay * moving_var[c] + (1.f - decay) * (float)uv;
    }
}

// eval-mode BN: moving statistics -> (scale, shift)
__global__ __launch_bounds__(256) void bn_eval_coeffs_kernel(int N, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta,
                                                             const float *__restrict__ mm,
                                                             const float *__restrict__ mv, float eps,
                                                             float *__restrict__ scale_o,
                                                             float *__restrict__ shift_o) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const float sc = gamma[c] * (1.0f / sqrtf(mv[c] + eps));
    scale_o[c] = sc;
    shift_o[c] = beta[c] - mm[c] * sc;
}

// backward BN: sums (sum G, sum G*Y) -> dgamma, dbeta and the dY = p*G + q*Y + t coefficient vectors
__global__ __launch_bounds__(256) void bn_bwd_coeffs_kernel(int N, double R, const double *__restrict__ ws,
                                                            const float *__restrict__ gamma,
                                                            const float *__restrict__ mean,
                                                            const float *__restrict__ rstd,
                                                            float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                            float *__restrict__ p_o, float *__restrict__ q_o,
                                                            float *__restrict__ t_o) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double sg = 0.0, sgy = 0.0;
    for (int s = 0; s < kRedSlices; ++s) {
        sg += ws[((long long)s * 2 + 0) * N + c];
        sgy += ws[((long long)s * 2 + 1) * N + c];
    }
    const double mu = mean[c], rs = rstd[c], g = gamma[c];
    const double dga = (sgy - mu * sg) * rs;
    const double p = g * rs;
    const double q = -p * rs * dga / R;
    const double t = -p * sg / R - q * mu;
    dgamma[c] = (float)dga;
    dbeta[c] = (float)sg;
    p_o[c] = (float)p;
    q_o[c] = (float)q;
    t_o[c] = (float)t;
}

// ---------------------------------------------------------------------------------------------
// out[g][c] = max_s relu(scale[c]*Y[g*S+s][c] + shift[c]); argmax = first s reaching it
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(long long G, int S, int C,
                                                              const float *__restrict__ Y,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ shift,
                                                              float *__restrict__ out,
                                                              unsigned char *__restrict__ argmax,
                                                              float *__restrict__ ysel) {
    const int c4n = C / 4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < G * c4n; e += (long long)gridDim.x * 256) {
        const long long g = e / c4n;
        const int c = (int)(e - g * c4n) * 4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float m[4] = {-1.f, -1.f, -1.f, -1.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f};
        int am[4] = {0, 0, 0, 0};
        const float *base = Y + (g * S) * C + c;
        for (int s = 0; s < S; ++s) {
            const float4 y = *reinterpret_cast<const float4 *>(base + (long long)s * C);
            const float a0 = fmaxf(fmaf(y.x, sc.x, sh.x), 0.f), a1 = fmaxf(fmaf(y.y, sc.y, sh.y), 0.f);
            const float a2 = fmaxf(fmaf(y.z, sc.z, sh.z), 0.f), a3 = fmaxf(fmaf(y.w, sc.w, sh.w), 0.f);
            if (a0 > m[0]) { m[0] = a0; am[0] = s; ys[0] = y.x; }
            if (a1 > m[1]) { m[1] = a1; am[1] = s; ys[1] = y.y; }
            if (a2 > m[2]) { m[2] = a2; am[2] = s; ys[2] = y.z; }
            if (a3 > m[3]) { m[3] = a3; am[3] = s; ys[3] = y.w; }
        }
        *reinterpret_cast<float4 *>(out + g * C + c) = make_float4(m[0], m[1], m[2], m[3]);
        if (argmax) {
            uchar4 q;
            q.x = (unsigned char)am[0]; q.y = (unsigned char)am[1];
            q.z = (unsigned char)am[2]; q.w = (unsigned char)am[3];
            *reinterpret_cast<uchar4 *>(argmax + g * C + c) = q;
        }
        if (ysel) *reinterpret_cast<float4 *>(ysel + g * C + c) = make_float4(ys[0], ys[1], ys[2], ys[3]);
    }
}

// the same over COMPACTED rows: group g owns rows 16 bstart[g] .. 16 bstart[g+1] - 1 (its real members followed by
// copies of member 0 up to the block boundary; the first maximiser wins, so a copy is never the arg-max)
__global__ __launch_bounds__(256) void bn_relu_maxpool_rows_kernel(long long G, int C, const float *__restrict__ Y,
                                                                   const float *__restrict__ scale,
                                                                   const float *__restrict__ shift,
                                                                   const int *__restrict__ bstart,
                                                                   float *__restrict__ out,
                                                                   unsigned char *__restrict__ argmax,
                                                                   float *__restrict__ ysel) {
    const int c4n = C / 4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < G * c4n; e += (long long)gridDim.x * 256) {
        const long long g = e / c4n;
        const int c = (int)(e - g * c4n) * 4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float m[4] = {-1.f, -1.f, -1.f, -1.f};
        float ys[4] = {0.f, 0.f, 0.f, 0.f};
        int am[4] = {0, 0, 0, 0};
        const long long r0 = (long long)bstart[g] * kBlk;
        const int S = (bstart[g + 1] - bstart[g]) * kBlk;
        const float *base = Y + r0 * C + c;
        // S is a multiple of 16: eight rows are requested before the first is looked at (a row-at-a-time loop has ONE
        // 16-byte load in flight per lane and spends 93 % of its wave cycles in s_waitcnt)
        for (int s0 = 0; s0 < S; s0 += 8) {
            float4 yv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) yv[u] = *reinterpret_cast<const float4 *>(base + (long long)(s0 + u) * C);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 y = yv[u];
                const int s = s0 + u;
                const float a0 = fmaxf(fmaf(y.x, sc.x, sh.x), 0.f), a1 = fmaxf(fmaf(y.y, sc.y, sh.y), 0.f);
                const float a2 = fmaxf(fmaf(y.z, sc.z, sh.z), 0.f), a3 = fmaxf(fmaf(y.w, sc.w, sh.w), 0.f);
                if (a0 > m[0]) { m[0] = a0; am[0] = s; ys[0] = y.x; }
                if (a1 > m[1]) { m[1] = a1; am[1] = s; ys[1] = y.y; }
                if (a2 > m[2]) { m[2] = a2; am[2] = s; ys[2] = y.z; }
                if (a3 > m[3]) { m[3] = a3; am[3] = s; ys[3] = y.w; }
            }
        }
        *reinterpret_cast<float4 *>(out + g * C + c) = make_float4(m[0], m[1], m[2], m[3]);
        if (argmax) {
            uchar4 q;
            q.x = (unsigned char)am[0]; q.y = (unsigned char)am[1];
            q.z = (unsigned char)am[2]; q.w = (unsigned char)am[3];
            *reinterpret_cast<uchar4 *>(argmax + g * C + c) = q;
        }
        if (ysel) *reinterpret_cast<float4 *>(ysel + g * C + c) = make_float4(ys[0], ys[1], ys[2], ys[3]);
    }
}

// compacted rows: per group the best of its blocks' partial extrema (written by the fused epilogue per 16-row block:
// the selected raw value and its row-in-group); sign(gamma) decides between max and min, the first block wins ties
// (blocks are in row order) -> ysel, arg-max, out = relu(scale * ysel + shift)
__global__ __launch_bounds__(256) void pool_combine_rows_kernel(long long total, int C, const float *__restrict__ ypart,
                                                                const unsigned char *__restrict__ ppart,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ scale,
                                                                const float *__restrict__ shift,
                                                                const int *__restrict__ bstart, float *__restrict__ out,
                                                                unsigned char *__restrict__ argmax,
                                                                float *__restrict__ ysel) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long g = e / C;
        const int c = (int)(e - g * C);
        const float sg = gamma[c] < 0.f ? -1.f : 1.f;
        const int b0 = bstart[g], b1 = bstart[g + 1];
        float best = ypart[(long long)b0 * C + c];
        int arg = ppart[(long long)b0 * C + c];
        for (int bk = b0 + 1; bk < b1; ++bk) {
            const float y = ypart[(long long)bk * C + c];
            if (y * sg > best * sg) { best = y; arg = ppart[(long long)bk * C + c]; }
        }
        out[e] = fmaxf(fmaf(best, scale[c], shift[c]), 0.f);
        if (argmax) argmax[e] = (unsigned char)arg;
        if (ysel) ysel[e] = best;
    }
}

// pooled output from the fused epilogue's selected raw values: out = relu(scale * ysel + shift)
__global__ __launch_bounds__(256) void pool_select_kernel(long long total, int C, const float *__restrict__ ysel,
                                                          const float *__restrict__ scale,
                                                          const float *__restrict__ shift, float *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C);
        out[e] = fmaxf(fmaf(ysel[e], scale[c], shift[c]), 0.f);
    }
}

// the two BN-backward sums of a max-pooled layer from (gpool, y at the selected row): stats [P][2][C];
// one workgroup per `groups_per_block` groups, threads = (row lane, column quad), 16-byte loads
__global__ __launch_bounds__(256) void pool_bwd_stats_sel_kernel(long long G, int C, const float *__restrict__ gpool,
                                                                 const float *__restrict__ ysel,
                                                                 const float *__restrict__ scale,
                                                                 const float *__restrict__ shift,
                                                                 float *__restrict__ stats, int groups_per_block,
                                                                 float *__restrict__ gmasked) {
    extern __shared__ float sm[];                     // [RL][2][C]
    const int c4n = C / 4;
    const int RL = c4n >= 256 ? 1 : 256 / c4n;
    const int rl = c4n >= 256 ? 0 : threadIdx.x / c4n;
    const long long g0 = (long long)blockIdx.x * groups_per_block;
    const long long g1 = min(G, g0 + groups_per_block);
    for (int cq = threadIdx.x % (c4n >= 256 ? 256 : c4n); cq < c4n; cq += 256) {
        const int c = cq * 4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
        if (rl < RL)
            for (long long g = g0 + rl; g < g1; g += RL) {
                const float4 y = *reinterpret_cast<const float4 *>(ysel + g * C + c);
                const float4 gp = *reinterpret_cast<const float4 *>(gpool + g * C + c);
                const float gm0 = fmaf(y.x, sc.x, sh.x) > 0.f ? gp.x : 0.f;
                const float gm1 = fmaf(y.y, sc.y, sh.y) > 0.f ? gp.y : 0.f;
                const float gm2 = fmaf(y.z, sc.z, sh.z) > 0.f ? gp.z : 0.f;
                const float gm3 = fmaf(y.w, sc.w, sh.w) > 0.f ? gp.w : 0.f;
                if (gmasked) *reinterpret_cast<float4 *>(gmasked + g * C + c) = make_float4(gm0, gm1, gm2, gm3);
                a1[0] += gm0; a1[1] += gm1; a1[2] += gm2; a1[3] += gm3;
                a2[0] = fmaf(gm0, y.x, a2[0]); a2[1] = fmaf(gm1, y.y, a2[1]);
                a2[2] = fmaf(gm2, y.z, a2[2]); a2[3] = fmaf(gm3, y.w, a2[3]);
            }
        if (rl < RL) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sm[(rl * 2 + 0) * C + c + e] = a1[e];
                sm[(rl * 2 + 1) * C + c + e] = a2[e];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int which = i / C, c = i % C;
        float t = 0.f;
        for (int l = 0; l < RL; ++l) t += sm[(l * 2 + which) * C + c];
        stats[((long long)blockIdx.x * 2 + which) * C + c] = t;
    }
}

// ... of a pooled gradient that arrives in TWO pieces and / or strided (an EdgeConv output that feeds the next layer and a column
// block of the concatenation, dgcnn.py:39-81: autograd's sum was a 134 MB launch of its own, a strided piece a copy): the pieces
// are added while the sums are taken and leave as ONE contiguous tensor gsum [G][C] for the data-gradient kernel behind
__global__ __launch_bounds__(256) void pool_bwd_stats_sum_kernel(long long G, int C, const float *__restrict__ ga, long long lda,
                                                                 const float *__restrict__ gb, long long ldb,
                                                                 const float *__restrict__ ysel,
                                                                 const float *__restrict__ scale,
                                                                 const float *__restrict__ shift,
                                                                 float *__restrict__ stats, int groups_per_block,
                                                                 float *__restrict__ gsum) {
    extern __shared__ float sm[];                     // [RL][2][C]
    const int c4n = C / 4;
    const int RL = c4n >= 256 ? 1 : 256 / c4n;
    const int rl = c4n >= 256 ? 0 : threadIdx.x / c4n;
    const long long g0 = (long long)blockIdx.x * groups_per_block;
    const long long g1 = min(G, g0 + groups_per_block);
    for (int cq = threadIdx.x % (c4n >= 256 ? 256 : c4n); cq < c4n; cq += 256) {
        const int c = cq * 4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
        if (rl < RL)
            for (long long g = g0 + rl; g < g1; g += RL) {
                const float4 y = *reinterpret_cast<const float4 *>(ysel + g * C + c);
                float4 gp = *reinterpret_cast<const float4 *>(ga + g * lda + c);
                if (gb) {
                    const float4 g2 = *reinterpret_cast<const float4 *>(gb + g * ldb + c);
                    gp.x += g2.x; gp.y += g2.y; gp.z += g2.z; gp.w += g2.w;
                }
                *reinterpret_cast<float4 *>(gsum + g * C + c) = gp;
                const float gm0 = fmaf(y.x, sc.x, sh.x) > 0.f ? gp.x : 0.f;
                const float gm1 = fmaf(y.y, sc.y, sh.y) > 0.f ? gp.y : 0.f;
                const float gm2 = fmaf(y.z, sc.z, sh.z) > 0.f ? gp.z : 0.f;
                const float gm3 = fmaf(y.w, sc.w, sh.w) > 0.f ? gp.w : 0.f;
                a1[0] += gm0; a1[1] += gm1; a1[2] += gm2; a1[3] += gm3;
                a2[0] = fmaf(gm0, y.x, a2[0]); a2[1] = fmaf(gm1, y.y, a2[1]);
                a2[2] = fmaf(gm2, y.z, a2[2]); a2[3] = fmaf(gm3, y.w, a2[3]);
            }
        if (rl < RL) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sm[(rl * 2 + 0) * C + c + e] = a1[e];
                sm[(rl * 2 + 1) * C + c + e] = a2[e];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int which = i / C, c = i % C;
        float t = 0.f;
        for (int l = 0; l < RL; ++l) t += sm[(l * 2 + which) * C + c];
        stats[((long long)blockIdx.x * 2 + which) * C + c] = t;
    }
}

// A[r][c] = relu(scale[c]*Y[r][c] + shift[c])   (stack output without pooling)
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(long long total4, int C,
                                                            const float *__restrict__ Y,
                                                            const float *__restrict__ scale,
                                                            const float *__restrict__ shift,
                                                            float *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long long)gridDim.x * 256) {
        const int c = (int)((e * 4) % C);
        const float4 y = reinterpret_cast<const float4 *>(Y)[e];
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float4 o;
        o.x = fmaxf(fmaf(y.x, sc.x, sh.x), 0.f);
        o.y = fmaxf(fmaf(y.y, sc.y, sh.y), 0.f);
        o.z = fmaxf(fmaf(y.z, sc.z, sh.z), 0.f);
        o.w = fmaxf(fmaf(y.w, sc.w, sh.w), 0.f);
        reinterpret_cast<float4 *>(out)[e] = o;
    }
}

// backward of relu(bn(Y)) for a materialised upstream grad Gout: Gm = Gout*[a>0], partial sums
// (sum Gm, sum Gm*Y) per 128-row tile: stats [P][2][C]
__global__ __launch_bounds__(256) void relu_mask_stats_kernel(long long R, int C, const float *__restrict__ Gout,
                                                              const float *__restrict__ Y,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ shift,
                                                              float *__restrict__ Gm, float *__restrict__ stats,
                                                              int rows_per_block) {
    // block: 256 threads = (C/4 column-quads) x (256/(C/4)) row lanes ... generic: thread owns column quad
    // cq = tid % c4n and strides rows by 256 / c4n; requires c4n <= 256 and 256 % c4n == 0 or loops columns.
    extern __shared__ float sm[];  // [rl][2][C]
    const int c4n = C / 4;
    const int rl = max(1, 256 / c4n);  // row lanes
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = min(R, r0 + rows_per_block);
    for (int cq = threadIdx.x % min(c4n, 256); cq < c4n; cq += 256) {
        const int c = cq * 4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c);
        float a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
        const int lane_r = (c4n >= 256) ? 0 : threadIdx.x / c4n;
        if (lane_r < rl) {
            for (long long r = r0 + lane_r; r < r1; r += rl) {
                const float4 g = *reinterpret_cast<const float4 *>(Gout + r * C + c);
                const float4 y = *reinterpret_cast<const float4 *>(Y + r * C + c);
                float4 o;
                o.x = fmaf(y.x, sc.x, sh.x) > 0.f ? g.x : 0.f;
                o.y = fmaf(y.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
                o.z = fmaf(y.z, sc.z, sh.z) > 0.f ? g.z : 0.f;
                o.w = fmaf(y.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
                *reinterpret_cast<float4 *>(Gm + r * C + c) = o;
                a1[0] += o.x; a1[1] += o.y; a1[2] += o.z; a1[3] += o.w;
                a2[0] = fmaf(o.x, y.x, a2[0]); a2[1] = fmaf(o.y, y.y, a2[1]);
                a2[2] = fmaf(o.z, y.z, a2[2]); a2[3] = fmaf(o.w, y.w, a2[3]);
            }
            for (int e = 0; e < 4; ++e) {
                sm[(lane_r * 2 + 0) * C + c + e] = a1[e];
                sm[(lane_r * 2 + 1) * C + c + e] = a2[e];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int which = i / C, c = i % C;
        float t = 0.f;
        for (int l = 0; l < rl; ++l) t += sm[(l * 2 + which) * C + c];
        stats[((long long)blockIdx.x * 2 + which) * C + c] = t;
    }
}

// sum partials [P][L] -> out[L] (deterministic): 64 consecutive elements x 4 partial lanes per workgroup
__global__ __launch_bounds__(256) void sum_partials_kernel(int P, long long L, const float *__restrict__ part,
                                                           float *__restrict__ out) {
    __shared__ double sm[4][64];
    const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + c;
    double s = 0.0;
    if (i < L)
        for (int p = pl; p < P; p += 4) s += (double)part[(long long)p * L + i];
    sm[pl][c] = s;
    __syncthreads();
    if (pl == 0 && i < L) out[i] = (float)((sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]));
}

// two adjacent reductions in one launch: blocks [0, ceil(L/64)) sum part -> out, the rest sum part2 -> out2
__global__ __launch_bounds__(1024) void sum_partials2_kernel(int P, long long L, const float *__restrict__ part,
                                                             float *__restrict__ out, long long L2,
                                                             const float *__restrict__ part2,
                                                             float *__restrict__ out2) {
    __shared__ double sm[16][64];
    const long long nb1 = (L + 63) / 64;
    const bool second = (long long)blockIdx.x >= nb1;
    const long long len = second ? L2 : L;
    const float *src = second ? part2 : part;
    float *dst = second ? out2 : out;
    const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const long long i = ((long long)blockIdx.x - (second ? nb1 : 0)) * 64 + c;
    double s = 0.0;
    if (i < len)
        for (int p = pl; p < P; p += 16) s += (double)src[(long long)p * len + i];
    sm[pl][c] = s;
    __syncthreads();
    if (pl == 0 && i < len) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sm[k][c];
        dst[i] = (float)t;
    }
}

// Wt[n][k] = W[k][n]
__global__ __launch_bounds__(256) void transpose_kernel(int K, int N, const float *__restrict__ W,
                                                        float *__restrict__ Wt) {
    __shared__ float t[32][33];
    const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (k0 + i < K && n0 + tx < N) t[i][tx] = W[(long long)(k0 + i) * N + n0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (n0 + i < N && k0 + tx < K) Wt[(long long)(n0 + i) * K + k0 + tx] = t[tx][i];
}

// few partial rows (P <= kFusedRows): column reduction and the per-channel finalisation in ONE launch.
// block = 32 columns x 32 row lanes; the row-lane totals meet in LDS in a fixed order (deterministic)
constexpr int kFusedRows = 1024;

__device__ __forceinline__ bool fused_col_sums(int P, int N, const float *__restrict__ part, double &s1, double &s2,
                                               int &c) {
    __shared__ double sm[2][32][32];
    c = blockIdx.x * 32 + (threadIdx.x & 31);
    const int g = threadIdx.x >> 5;
    double a1 = 0.0, a2 = 0.0;
    if (c < N)
        for (int p = g; p < P; p += 32) {
            a1 += (double)part[((long long)p * 2 + 0) * N + c];
            a2 += (double)part[((long long)p * 2 + 1) * N + c];
        }
    sm[0][g][threadIdx.x & 31] = a1;
    sm[1][g][threadIdx.x & 31] = a2;
    __syncthreads();
    if (g != 0 || c >= N) return false;
    s1 = s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) { s1 += sm[0][i][threadIdx.x]; s2 += sm[1][i][threadIdx.x]; }
    return true;
}

__global__ __launch_bounds__(1024) void bn_finalize_fused_kernel(int P, int N, double R, const float *__restrict__ part,
                                                                const float *__restrict__ pivot,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float eps,
                                                                float decay, int unbiased,
                                                                float *__restrict__ moving_mean,
                                                                float *__restrict__ moving_var,
                                                                float *__restrict__ mean_o,
                                                                float *__restrict__ rstd_o,
                                                                float *__restrict__ scale_o,
                                                                float *__restrict__ shift_o) {
    double s1, s2;
    int c;
    if (!fused_col_sums(P, N, part, s1, s2, c)) return;
    const double dm = s1 / R;                                    // sums of (y - pivot), (y - pivot)^2: see bn_finalize_kernel
    const double mean = dm + (pivot ? (double)pivot[c] : 0.0);
    double var = s2 / R - dm * dm;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * rstd;
    mean_o[c] = (float)mean;
    rstd_o[c] = rstd;
    scale_o[c] = sc;
    shift_o[c] = beta[c] - (float)mean * sc;
    if (moving_mean) {
        const double uv = (unbiased && R > 1.0) ? var * (R / (R - 1.0)) : var;
        moving_mean[c] = decay * moving_mean[c] + (1.f - decay) * (float)mean;
        moving_var[c] = decay * moving_var[c] + (1.f - decay) * (float)uv;
    }
}

__global__ __launch_bounds__(1024) void bn_bwd_coeffs_fused_kernel(int P, int N, double R,
                                                                  const float *__restrict__ part,
                                                                  const float *__restrict__ gamma,
                                                                  const float *__restrict__ mean,
                                                                  const float *__restrict__ rstd,
                                                                  float *__restrict__ dgamma,
                                                                  float *__restrict__ dbeta, float *__restrict__ p_o,
                                                                  float *__restrict__ q_o, float *__restrict__ t_o) {
    double sg, sgy;
    int c;
    if (!fused_col_sums(P, N, part, sg, sgy, c)) return;
    const double mu = mean[c], rs = rstd[c], g = gamma[c];
    const double dga = (sgy - mu * sg) * rs;
    const double p = g * rs;
    const double q = -p * rs * dga / R;
    const double t = -p * sg / R - q * mu;
    dgamma[c] = (float)dga;
    dbeta[c] = (float)sg;
    p_o[c] = (float)p;
    q_o[c] = (float)q;
    t_o[c] = (float)t;
}

int reduce_stats(int P, int N, const float *part, double *ws, hipStream_t st) {
    hipLaunchKernelGGL(colreduce_stage1, dim3((N + 31) / 32, 2, kRedSlices), dim3(256), 0, st, P, N, part, ws);
    return pcops_launch_status();
}

}  // namespace
}  // namespace pcops_mlp
using namespace pcops_mlp;

// the sum of partial copies for the other translation units of the family (common.h): one block per 64 elements of out, then of out2
int pcops_mlp_sum_partials2(int P, long long L, const float *part, float *out, long long L2, const float *part2, float *out2,
                            hipStream_t st) {
    hipLaunchKernelGGL(sum_partials2_kernel, dim3(cdiv(L, 64) + (out2 ? cdiv(L2, 64) : 0)), dim3(1024), 0, st, P, L, part, out,
                       L2, part2, out2);
    return pcops_launch_status();
}

extern "C" {

unsigned long long pcops_mlp_reduce_workspace_bytes(int N) {
    return (unsigned long long)kRedSlices * 2 * (unsigned long long)N * sizeof(double);
}

int pcops_mlp_pool_combine_rows(long long G, int C, const float *ypart, const unsigned char *ppart,
                                const float *gamma, const float *scale, const float *shift,
                                const pcops_rows_t *rows, float *out, unsigned char *argmax, float *ysel,
                                pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 0 && C >= 1);
    if (G == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(ypart); PCOPS_REQUIRE_PTR(ppart); PCOPS_REQUIRE_PTR(gamma); PCOPS_REQUIRE_PTR(scale);
    PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(out); PCOPS_REQUIRE_PTR(rows);
    const int rrc = rows_ok(rows);
    if (rrc) return rrc;
    const long long total = G * C;
    const unsigned grid = cdiv(total, 256) < 16384u ? cdiv(total, 256) : 16384u;
    hipLaunchKernelGGL(pool_combine_rows_kernel, dim3(grid), dim3(256), 0, as_stream(stream), total, C, ypart, ppart,
                       gamma, scale, shift, rows->block_start, out, argmax, ysel);
    return pcops_launch_status();
}

int pcops_mlp_pool_select(long long G, int C, const float *ysel, const float *scale, const float *shift,
                          float *out, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 0 && C >= 1);
    if (G == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(out);
    const long long total = G * C;
    const unsigned grid = cdiv(total, 256) < 16384u ? cdiv(total, 256) : 16384u;
    hipLaunchKernelGGL(pool_select_kernel, dim3(grid), dim3(256), 0, as_stream(stream), total, C, ysel, scale,
                       shift, out);
    return pcops_launch_status();
}

int pcops_mlp_bn_finalize(int P, int N, long long R, const float *stats_partial, const float *stat_pivot,
                          void *workspace, const float *gamma, const float *beta, float eps, float decay,
                          int unbiased_moving_var, float *moving_mean, float *moving_var, float *mean,
                          float *rstd, float *scale, float *shift, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(P >= 1 && N >= 1 && R >= 1);
    PCOPS_REQUIRE_PTR(stats_partial); PCOPS_REQUIRE_PTR(workspace); PCOPS_REQUIRE_PTR(gamma);
    PCOPS_REQUIRE_PTR(beta); PCOPS_REQUIRE_PTR(mean); PCOPS_REQUIRE_PTR(rstd); PCOPS_REQUIRE_PTR(scale);
    PCOPS_REQUIRE_PTR(shift);
    PCOPS_REQUIRE_ARG((moving_mean == nullptr) == (moving_var == nullptr));
    hipStream_t st = as_stream(stream);
    if (P <= kFusedRows) {
        hipLaunchKernelGGL(bn_finalize_fused_kernel, dim3((N + 31) / 32), dim3(1024), 0, st, P, N, (double)R,
                           stats_partial, stat_pivot, gamma, beta, eps, decay, unbiased_moving_var, moving_mean, moving_var, mean,
                           rstd, scale, shift);
        return pcops_launch_status();
    }
    double *ws = static_cast<double *>(workspace);
    int rc = reduce_stats(P, N, stats_partial, ws, st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, (double)R, ws, stat_pivot,
                       gamma, beta, eps, decay, unbiased_moving_var, moving_mean, moving_var, mean, rstd, scale, shift);
    return pcops_launch_status();
}

int pcops_mlp_bn_eval_coeffs(int N, const float *gamma, const float *beta, const float *moving_mean,
                             const float *moving_var, float eps, float *scale, float *shift,
                             pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(N >= 1);
    PCOPS_REQUIRE_PTR(gamma); PCOPS_REQUIRE_PTR(beta); PCOPS_REQUIRE_PTR(moving_mean);
    PCOPS_REQUIRE_PTR(moving_var); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift);
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), N, gamma,
                       beta, moving_mean, moving_var, eps, scale, shift);
    return pcops_launch_status();
}

int pcops_mlp_bn_relu_maxpool(long long G, int S, int C, const float *Y, const float *scale,
                              const float *shift, float *out, unsigned char *argmax, float *ysel,
                              pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 0 && S >= 1 && S <= 256 && C >= 4 && C % 4 == 0);
    if (G == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(out);
    const long long total = G * (C / 4);
    const unsigned grid = cdiv(total, 256) < 32768u ? cdiv(total, 256) : 32768u;
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(grid), dim3(256), 0, as_stream(stream), G, S, C, Y, scale,
                       shift, out, argmax, ysel);
    return pcops_launch_status();
}

int pcops_mlp_bn_relu_maxpool_rows(long long G, int C, const float *Y, const float *scale, const float *shift,
                                   const pcops_rows_t *rows, float *out, unsigned char *argmax, float *ysel,
                                   pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 0 && C >= 4 && C % 4 == 0);
    if (G == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(out);
    PCOPS_REQUIRE_PTR(rows);
    const int rrc = rows_ok(rows);
    if (rrc) return rrc;
    const long long total = G * (C / 4);
    const unsigned grid = cdiv(total, 256) < 32768u ? cdiv(total, 256) : 32768u;
    hipLaunchKernelGGL(bn_relu_maxpool_rows_kernel, dim3(grid), dim3(256), 0, as_stream(stream), G, C, Y, scale,
                       shift, rows->block_start, out, argmax, ysel);
    return pcops_launch_status();
}

int pcops_mlp_bn_relu_apply(long long R, int C, const float *Y, const float *scale, const float *shift,
                            float *out, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(R >= 0 && C >= 4 && C % 4 == 0);
    if (R == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(out);
    const long long total4 = R * C / 4;
    const unsigned grid = cdiv(total4, 256) < 32768u ? cdiv(total4, 256) : 32768u;
    hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(grid), dim3(256), 0, as_stream(stream), total4, C, Y, scale,
                       shift, out);
    return pcops_launch_status();
}

// ---- backward ---------------------------------------------------------------------------------
int pcops_mlp_bwd_stats_rows(long long R) { return (int)((R + 511) / 512); }
int pcops_mlp_bwd_pool_stats_rows(long long G) { return (int)((G + 15) / 16); }

/* Gm = Gout * [relu(bn(Y)) > 0]; partial sums (sum Gm, sum Gm*Y) -> stats [pcops_mlp_bwd_stats_rows(R)][2][C] */
int pcops_mlp_relu_mask_stats(long long R, int C, const float *Gout, const float *Y, const float *scale,
                              const float *shift, float *Gm, float *stats_partial, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(R >= 1 && C >= 4 && C % 4 == 0);
    PCOPS_REQUIRE_PTR(Gout); PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(scale); PCOPS_REQUIRE_PTR(shift);
    PCOPS_REQUIRE_PTR(Gm); PCOPS_REQUIRE_PTR(stats_partial);
    const int c4n = C / 4;
    PCOPS_REQUIRE_SHAPE(c4n >= 256 || 256 % c4n == 0);
    const int rl = c4n >= 256 ? 1 : 256 / c4n;
    const size_t lds = (size_t)rl * 2 * C * sizeof(float);
    if (lds > 64 * 1024) return PCOPS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(relu_mask_stats_kernel, dim3(pcops_mlp_bwd_stats_rows(R)), dim3(256), lds,
                       as_stream(stream), R, C, Gout, Y, scale, shift, Gm, stats_partial, 512);
    return pcops_launch_status();
}

int pcops_mlp_pool_bwd_stats(long long G, int C, const float *gpool, const float *ysel, const float *scale,
                             const float *shift, float *stats_partial, float *gmasked, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 1 && C >= 4 && C % 4 == 0);
    PCOPS_REQUIRE_PTR(gpool); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(scale);
    PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(stats_partial);
    const int c4n = C / 4;
    const int rl = c4n >= 256 ? 1 : 256 / c4n;        // threads beyond rl * c4n idle when c4n does not divide 256
    const size_t lds = (size_t)rl * 2 * C * sizeof(float);
    if (lds > 64 * 1024) return PCOPS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pool_bwd_stats_sel_kernel, dim3(pcops_mlp_bwd_pool_stats_rows(G)), dim3(256), lds,
                       as_stream(stream), G, C, gpool, ysel, scale, shift, stats_partial, 16, gmasked);
    return pcops_launch_status();
}

int pcops_mlp_pool_bwd_stats_sum(long long G, int C, const float *ga, long long lda, const float *gb, long long ldb,
                                 const float *ysel, const float *scale, const float *shift, float *stats_partial,
                                 float *gsum, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(G >= 1 && C >= 4 && C % 4 == 0 && lda >= C && lda % 4 == 0 && (!gb || (ldb >= C && ldb % 4 == 0)));
    PCOPS_REQUIRE_PTR(ga); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(scale);
    PCOPS_REQUIRE_PTR(shift); PCOPS_REQUIRE_PTR(stats_partial); PCOPS_REQUIRE_PTR(gsum);
    PCOPS_REQUIRE_ARG(((uintptr_t)ga | (uintptr_t)gb | (uintptr_t)gsum) % 16 == 0);
    const int c4n = C / 4;
    const int rl = c4n >= 256 ? 1 : 256 / c4n;
    const size_t lds = (size_t)rl * 2 * C * sizeof(float);
    if (lds > 64 * 1024) return PCOPS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pool_bwd_stats_sum_kernel, dim3(pcops_mlp_bwd_pool_stats_rows(G)), dim3(256), lds,
                       as_stream(stream), G, C, ga, lda, gb, ldb, ysel, scale, shift, stats_partial, 16, gsum);
    return pcops_launch_status();
}

int pcops_mlp_bn_bwd_coeffs(int P, int N, long long R, const float *stats_partial, void *workspace,
                            const float *gamma, const float *mean, const float *rstd, float *dgamma,
                            float *dbeta, float *p, float *q, float *t, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(P >= 1 && N >= 1 && R >= 1);
    PCOPS_REQUIRE_PTR(stats_partial); PCOPS_REQUIRE_PTR(workspace); PCOPS_REQUIRE_PTR(gamma);
    PCOPS_REQUIRE_PTR(mean); PCOPS_REQUIRE_PTR(rstd); PCOPS_REQUIRE_PTR(dgamma); PCOPS_REQUIRE_PTR(dbeta);
    PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(q); PCOPS_REQUIRE_PTR(t);
    hipStream_t st = as_stream(stream);
    if (P <= kFusedRows) {
        hipLaunchKernelGGL(bn_bwd_coeffs_fused_kernel, dim3((N + 31) / 32), dim3(1024), 0, st, P, N, (double)R,
                           stats_partial, gamma, mean, rstd, dgamma, dbeta, p, q, t);
        return pcops_launch_status();
    }
    double *ws = static_cast<double *>(workspace);
    int rc = reduce_stats(P, N, stats_partial, ws, st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_bwd_coeffs_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, (double)R, ws, gamma,
                       mean, rstd, dgamma, dbeta, p, q, t);
    return pcops_launch_status();
}

int pcops_mlp_transpose(int K, int N, const float *W, float *Wt, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(K >= 1 && N >= 1);
    PCOPS_REQUIRE_PTR(W); PCOPS_REQUIRE_PTR(Wt);
    hipLaunchKernelGGL(transpose_kernel, dim3((N + 31) / 32, (K + 31) / 32), dim3(256), 0, as_stream(stream), K, N,
                       W, Wt);
    return pcops_launch_status();
}

}  // extern "C"
