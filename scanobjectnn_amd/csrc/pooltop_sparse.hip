// pooltop_sparse.hip -- the algebraic backward of a pooled top layer (pcops.h "algebraic backward of a pooled top layer"): what
// is not a matrix product.  The dense halves are mlp.hip's (pcops_mlp_gemm_dgrad_top, pcops_mlp_gram) and small_gemm.hip's;
// pooltop_groups.hip has the form for small uncompacted groups that never writes an addend.  Here:
//
//   pool_top_prep / pool_top_finish   the layer's small operands (W^T, W diag(q), u, v) and the closing sums of dW and db
//   pool_top_addend*, pool_top_wsparse*   the sparse halves -- the arg-max rows' share of dX and of dW -- over whole groups,
//                                     and over compacted rows plain and software-pipelined (the algebra: further down)
//   dy_apply                          dY = (t + p.G) + q.Y as a tensor
// The shape queries that ask the product planners (pcops_mlp_pool_top_supported, pcops_mlp_pool_top_rows_supported) are
// mlp.hip's; the launchers here call them through the C ABI.  Three kernels keep the namespace they had in mlp.hip
// (pcops_mlp::(anonymous namespace)::...), the others the global one: the profiles know them by those names.
#include "common.h"

namespace pcops_mlp {
namespace {

// dY = (t + p.G) + q.Y over whole rows (the data gradient of a first layer whose "gather" is the identity: the whole-cloud
// group of sample_and_group_all, pointnet_util.py:59-84) -- it was an addcmul and an in-place addcmul over the tensor
__global__ __launch_bounds__(256) void dy_apply_kernel(long long total4, int N4, const float4 *__restrict__ G,
                                                       const float4 *__restrict__ Y, const float4 *__restrict__ p,
                                                       const float4 *__restrict__ q, const float4 *__restrict__ t,
                                                       float4 *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % N4);
        const float4 g = G[e], y = Y[e], pp = p[c], qq = q[c], tt = t[c];
        out[e] = make_float4((tt.x + g.x * pp.x) + y.x * qq.x, (tt.y + g.y * pp.y) + y.y * qq.y,
                             (tt.z + g.z * pp.z) + y.z * qq.z, (tt.w + g.w * pp.w) + y.w * qq.w);
    }
}

// The algebraic top layer's small operands in ONE launch (they were a transpose, an elementwise product, an addcmul and a
// matrix-vector launch of the small-GEMM kernel):
//   Wt[n][k] = W[k][n],  Wq[k][n] = W[k][n] q[n],  u[n] = q[n] b[n] + t[n]  (tile row 0 writes u),
//   v[k] = sum_n W[k][n] u[n]  (the workgroups behind the tiles: eight rows each, a row per half-wave pair, lanes over n)
__global__ __launch_bounds__(256) void pool_top_prep_kernel(int K, int N, const float *__restrict__ W,
                                                            const float *__restrict__ b, const float *__restrict__ q,
                                                            const float *__restrict__ tt, float *__restrict__ Wt,
                                                            float *__restrict__ Wq, float *__restrict__ u,
                                                            float *__restrict__ v) {
    __shared__ float t[32][33];
    const int tiles_y = (K + 31) / 32;
    if ((int)blockIdx.y >= tiles_y) {                    // v: eight rows per workgroup, numbered along x then y
        if (v == nullptr) return;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int vb = ((int)blockIdx.y - tiles_y) * (int)gridDim.x + (int)blockIdx.x;
        for (int rr = 0; rr < 2; ++rr) {
            const int k = vb * 8 + wave * 2 + rr;
            if (k >= K) continue;                        // (wave-uniform)
            float acc = 0.f;
            for (int n = lane; n < N; n += 64) acc = fmaf(W[(long long)k * N + n], q[n] * b[n] + tt[n], acc);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (lane == 0) v[k] = acc;
        }
        return;
    }
    const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float qn = n0 + tx < N ? q[n0 + tx] : 0.f;
    for (int i = ty; i < 32; i += 8)
        if (k0 + i < K && n0 + tx < N) {
            const float w = W[(long long)(k0 + i) * N + n0 + tx];
            t[i][tx] = w;
            Wq[(long long)(k0 + i) * N + n0 + tx] = w * qn;
        }
    if (blockIdx.y == 0 && ty == 0 && n0 + tx < N) u[n0 + tx] = qn * b[n0 + tx] + tt[n0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (n0 + i < N && k0 + tx < K) Wt[(long long)(n0 + i) * K + k0 + tx] = t[tx][i];
}

// ... and the sums that close its weight and bias gradient (an in-place add, an outer product, six vector launches and the
// matrix-vector launch for xw = xsum^T W, which the first row of workgroups now adds up per column, k ascending):
//   dW[k][n] = (dW[k][n] + Ssp[k][n]) + xsum[k] u[n],   db[n] = (cfsum[n] + q[n] (xw[n] + R b[n])) + R t[n]
__global__ __launch_bounds__(256) void pool_top_finish_kernel(int K, int N, float R, float *__restrict__ dW,
                                                              const float *__restrict__ Ssp, const float *__restrict__ xsum,
                                                              const float *__restrict__ u, const float *__restrict__ cfsum,
                                                              const float *__restrict__ q, const float *__restrict__ W,
                                                              const float *__restrict__ b, const float *__restrict__ tt,
                                                              float *__restrict__ db) {
    if (blockIdx.y < 8) {
        // db: 32 columns per workgroup (block 8 x + y of the 256-column strip x), eight lanes of k per column, four chains each
        // (a column's K loads would otherwise wait on one another: 61 us for K = 512 with one thread per column)
        __shared__ float red[8][32];
        const int c = threadIdx.x & 31, kl = threadIdx.x >> 5;
        const int n = (blockIdx.x * 8 + blockIdx.y) * 32 + c;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (n < N) {
            int k = kl;
            for (; k + 24 < K; k += 32) {
                a0 = fmaf(xsum[k], W[(long long)k * N + n], a0);
                a1 = fmaf(xsum[k + 8], W[(long long)(k + 8) * N + n], a1);
                a2 = fmaf(xsum[k + 16], W[(long long)(k + 16) * N + n], a2);
                a3 = fmaf(xsum[k + 24], W[(long long)(k + 24) * N + n], a3);
            }
            for (; k < K; k += 8) a0 = fmaf(xsum[k], W[(long long)k * N + n], a0);
        }
        red[kl][c] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (kl == 0 && n < N) {
            const float xw = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + ((red[4][c] + red[5][c]) + (red[6][c] + red[7][c]));
            db[n] = (cfsum[n] + q[n] * (xw + R * b[n])) + R * tt[n];
        }
        return;
    }
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float un = u[n];
    const int kb = ((int)blockIdx.y - 8) * 8;
    for (int k = kb; k < min(K, kb + 8); ++k) {
        const long long e = (long long)k * N + n;
        dW[e] = (dW[e] + Ssp[e]) + xsum[k] * un;
    }
}

}  // namespace
}  // namespace pcops_mlp
using namespace pcops_mlp;

// ---------------------------------------------------------------------------------------------
// Algebraic backward of a POOLED top layer  Y = X W + b,  X = relu(bn(Yprev)),  out = max_group relu(bn(Y)).
// Its dY = p.G + q.Y + t has a DENSE part that is affine in X and a SPARSE part (one row per group and channel):
//   dX = (p.G) W^T + X (W diag(q) W^T) + 1 (W (q.b + t))^T
//   dW = X^T (p.G) + (X^T X) (W diag(q)) + (X^T 1) (q.b + t)^T
// so neither gradient needs Y, and the two big products shrink from K x N to K x K (N = 2K in every SA module, N = 3.2K
// .. 8K for the layers pooled over whole clouds).  The sparse parts are G x N row operations:
//   pool_top_addend_kernel   per group: arg-max rows -> compact addend rows  sum_c cf[c] Wt[c][:]  + the row -> slot map
//   pool_top_wsparse_kernel per channel: sum over the groups of cf X[arg row][:]
// cf[g][c] = p[c] gout[g][c] [relu(bn(ysel[g][c])) > 0].  Sums run in ascending channel / group order (deterministic).
template <int NT>      // threads: 1024 for few large groups (a wave set per segment needs the waves), 256 otherwise
__global__ __launch_bounds__(NT) void pool_top_addend_kernel(int S, int C, int Kp, int slots_per_group,
                                                              const float *__restrict__ gout,
                                                              const float *__restrict__ ysel,
                                                              const unsigned char *__restrict__ arg,
                                                              const float *__restrict__ sc, const float *__restrict__ sh,
                                                              const float *__restrict__ p, const float *__restrict__ Wt,
                                                              float *__restrict__ addend, int *__restrict__ rowmap) {
    // hit-driven: the (row, channel) pairs with a non-zero coefficient are compacted, sorted by (row, channel) with a
    // bitonic network in LDS (<= 1024 keys), cut into one segment per row, and a 16-lane set per segment adds the
    // segment's Wt rows in ascending channel order.  Work is O(hits log hits), not O(S C).
    __shared__ float cf[1024];
    __shared__ unsigned key[1024];                 // row << 10 | channel, 0xFFFFFFFF padding
    __shared__ int segstart[1025];                 // first sorted position of segment i
    __shared__ int wcount[16];
    constexpr int CPT = 1024 / NT, NW = NT / 64;     // channels per thread, waves
    const long long g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < S; s += NT) rowmap[g * S + s] = -1;
    // ---- coefficients and compaction of the hits (C <= 1024: four channels per thread)
    float v[CPT];
    unsigned row[CPT];
    unsigned long long hm[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = i * NT + tid;
        v[i] = 0.f;
        row[i] = 0;
        if (c < C) {
            const long long e = g * C + c;
            v[i] = fmaf(ysel[e], sc[c], sh[c]) > 0.f ? p[c] * gout[e] : 0.f;
            row[i] = arg[e];
            cf[c] = v[i];
        }
        hm[i] = __ballot(v[i] != 0.f);
        if (lane == 0) wcount[i * NW + wave] = __popcll(hm[i]);
        key[c] = 0xFFFFFFFFu;
    }
    __syncthreads();
    int nh = 0, base[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        for (int w = 0; w < NW; ++w) {
            if (w == wave) base[i] = nh;
            nh += wcount[i * NW + w];
        }
    if (nh == 0) return;                           // a chunk that won no channel (layers pooled over whole clouds)
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (v[i] != 0.f)
            key[base[i] + __popcll(hm[i] & ((1ull << lane) - 1ull))] = (row[i] << 10) | (unsigned)(i * NT + tid);
    int n2 = 64;
    while (n2 < nh) n2 <<= 1;
    // ---- bitonic sort of key[0 .. n2): n2 / 2 compare-exchanges per stage
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < n2 / 2; t += NT) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned a = key[lo], b = key[hi];
                if ((a > b) == ((lo & k) == 0)) { key[lo] = b; key[hi] = a; }
            }
        }
    __syncthreads();
    // ---- segments: a new one wherever the row changes (positions i * 256 + tid, i.e. ascending over (i, wave, lane))
    bool first[CPT];
    unsigned long long fm[CPT];
    unsigned mykey[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int pos = i * NT + tid;
        mykey[i] = pos < nh ? key[pos] : 0u;
        first[i] = pos < nh && (pos == 0 || (key[pos - 1] >> 10) != (mykey[i] >> 10));
        fm[i] = __ballot(first[i]);
    }
    __syncthreads();                               // wcount is reused
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < CPT; ++i) wcount[i * NW + wave] = __popcll(fm[i]);
    __syncthreads();
    int nseg = 0, sbase[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        for (int w = 0; w < NW; ++w) {
            if (w == wave) sbase[i] = nseg;
            nseg += wcount[i * NW + w];
        }
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (first[i]) {
            const int si = sbase[i] + __popcll(fm[i] & ((1ull << lane) - 1ull));
            segstart[si] = i * NT + tid;
            rowmap[g * S + (mykey[i] >> 10)] = (int)(g * slots_per_group) + si;
        }
    if (tid == 0) segstart[nseg] = nh;
    __syncthreads();
    // ---- a 16-lane set per segment; lane q of the set owns the float4 columns q, q + 16, ... of the Kp-wide row
    constexpr int KQ = 8;                          // Kp <= 512
    const int sub = lane >> 4, q = lane & 15;
    const int kq = (Kp + 63) / 64;
    for (int si = wave * 4 + sub; si < nseg; si += NW * 4) {
        const int e0 = segstart[si], e1 = segstart[si + 1];
        float4 acc[KQ];
#pragma unroll
        for (int i = 0; i < KQ; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e = e0; e < e1; ++e) {
            const int c = key[e] & 1023u;
            const float w = cf[c];
            const float *src = Wt + (long long)c * Kp;
#pragma unroll
            for (int i = 0; i < KQ; ++i) {
                const int k = (i * 16 + q) * 4;
                if (i < kq && k < Kp) {
                    const float4 wt = *reinterpret_cast<const float4 *>(src + k);
                    acc[i].x = fmaf(w, wt.x, acc[i].x); acc[i].y = fmaf(w, wt.y, acc[i].y);
                    acc[i].z = fmaf(w, wt.z, acc[i].z); acc[i].w = fmaf(w, wt.w, acc[i].w);
                }
            }
        }
        float *dst = addend + (g * slots_per_group + si) * (long long)Kp;
#pragma unroll
        for (int i = 0; i < KQ; ++i) {
            const int k = (i * 16 + q) * 4;
            if (i < kq && k < Kp) *reinterpret_cast<float4 *>(dst + k) = acc[i];
        }
    }
}

// one workgroup per channel c, its 4 waves take a quarter of the groups each:
//   Ssp[k][c] = sum_g cf[g][c] X[g S + arg[g][c]][k],  cfsum[c] = sum_g cf[g][c]      (wave partials added in order)
__global__ __launch_bounds__(256) void pool_top_wsparse_kernel(long long G, int S, int C, int Kp,
                                                               const float *__restrict__ gout,
                                                               const float *__restrict__ ysel,
                                                               const unsigned char *__restrict__ arg,
                                                               const float *__restrict__ sc, const float *__restrict__ sh,
                                                               const float *__restrict__ p,
                                                               const float *__restrict__ Yprev,
                                                               const float *__restrict__ psc, const float *__restrict__ psh,
                                                               float *__restrict__ Ssp, float *__restrict__ cfsum) {
    constexpr int KR = 8, U = 8;                                    // Kp <= 64 KR; hit rows in flight
    __shared__ float red[4][64 * KR + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x;
    const float scc = sc[c], shc = sh[c], pc = p[c];
    const int kr = (Kp + 63) / 64;                                  // registers in use (wave-uniform)
    float asc[KR], ash[KR], acc[KR];
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const int k = lane + 64 * i;
        asc[i] = (k < Kp && psc) ? psc[k] : 1.f;
        ash[i] = (k < Kp && psc) ? psh[k] : 0.f;
        acc[i] = 0.f;
    }
    float csum = 0.f;
    const long long gq = (G + 3) / 4;
    const long long gend = (wave + 1) * gq < G ? (wave + 1) * gq : G;
    for (long long g0 = wave * gq; g0 < gend; g0 += 64) {
        const long long g = g0 + lane;
        float cf = 0.f;
        int row = 0;
        if (g < gend) {
            const long long e = g * C + c;
            cf = fmaf(ysel[e], scc, shc) > 0.f ? pc * gout[e] : 0.f;
            row = arg[e];
        }
        unsigned long long hits = __ballot(cf != 0.f);
        while (hits) {                                              // wave-uniform: U hit groups at a time
            float w[U];
            long long r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                w[u] = 0.f;
                r[u] = 0;
                if (hits) {
                    const int l = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    w[u] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cf), l));
                    r[u] = (g0 + l) * S + __builtin_amdgcn_readlane(row, l);
                }
            }
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                if (i >= kr) break;
                const int k = lane + 64 * i;
                float x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) x[u] = (k < Kp) ? Yprev[r[u] * Kp + k] : 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float xv = psc ? fmaxf(fmaf(x[u], asc[i], ash[i]), 0.f) : x[u];
                    acc[i] = fmaf(w[u], xv, acc[i]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) csum += w[u];
        }
    }
#pragma unroll
    for (int i = 0; i < KR; ++i) red[wave][lane + 64 * i] = acc[i];
    if (lane == 0) red[wave][64 * KR] = csum;
    __syncthreads();
    for (int k = threadIdx.x; k < Kp; k += 256)
        Ssp[(long long)k * C + c] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    if (threadIdx.x == 0)
        cfsum[c] = (red[0][64 * KR] + red[1][64 * KR]) + (red[2][64 * KR] + red[3][64 * KR]);
}

// ---- the two sparse halves over COMPACTED rows, for MANY SMALL groups (the grouped stacks: 32 768 groups of <= 64 rows at
// the SSG config's second level).  The kernels above give a workgroup to a group / a channel and fetch a Kp-wide row of W^T /
// of X per hit through L2 -- 4.3 GB of 512-byte gathers each at that shape.  Here the reused operand sits in LDS:
//   pool_top_addend_rows_kernel   W^T [C][KP] resident (128 KB), persistent workgroups, four groups per round
//   pool_top_wsparse_rows_kernel  group-major: a group's rows of X (contiguous in the compacted stack) staged once
// The row of slot (g, a) is 16 block_start[g] + a; argmax is the row-in-group in compacted numbering.  Sums in a fixed order.
//
// addend (PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 0; 1 takes pool_top_addend_rows_pipe_kernel below): a quarter of the workgroup
// (256 threads = the C <= 256 channels) owns one group per round.  The channels that
// picked row r are a C-bit mask in LDS (integer OR: the result does not depend on the order); KP / 4 lanes per row then add
// cf[c] Wt[c][:] over the set bits in ascending channel order and write the row ONCE.  The addend is indexed by the
// compacted row itself (slot = row), rowmap [row] = row or -1.
template <int KP>
__global__ __launch_bounds__(1024) void pool_top_addend_rows_kernel(int G, int C, const float *__restrict__ gout,
                                                                    const float *__restrict__ ysel,
                                                                    const unsigned char *__restrict__ arg,
                                                                    const float *__restrict__ sc, const float *__restrict__ sh,
                                                                    const float *__restrict__ p, const float *__restrict__ Wt,
                                                                    const int *__restrict__ block_start,
                                                                    float *__restrict__ addend, int *__restrict__ rowmap) {
    constexpr int LPR = KP / 4, RPP = 256 / LPR;      // lanes per row (a float4 each), rows per pass of a quarter
    constexpr int MAXR = 128, MW = 8;                 // rows per group, mask words per row (C <= 256)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ws = lds;                                  // [C][KP]
    float *cf = Ws + (size_t)C * KP;                  // [4][256]
    unsigned *mask = reinterpret_cast<unsigned *>(cf + 4 * 256);      // [4][MAXR][MW]
    const int tid = threadIdx.x, sub = tid >> 8, c = tid & 255;
    for (int e = tid; e < C * (KP / 4); e += 1024)
        reinterpret_cast<float4 *>(Ws)[e] = reinterpret_cast<const float4 *>(Wt)[e];
    const float scc = c < C ? sc[c] : 0.f, shc = c < C ? sh[c] : 0.f, pc = c < C ? p[c] : 0.f;
    float *mycf = cf + sub * 256;
    unsigned *mymask = mask + sub * MAXR * MW;
    const int q = c % LPR, rsub = c / LPR;
    float v = 0.f;
    int row = 0, base = 0, nrows = 0;
    auto fetch = [&](long long g) {
        v = 0.f; row = 0; base = 0; nrows = 0;
        if (g < G) {
            const int b0 = block_start[g];
            base = kBlk * b0;
            nrows = kBlk * (block_start[g + 1] - b0);
            nrows = nrows < MAXR ? nrows : MAXR;
            if (c < C) {
                const long long e = g * C + c;
                v = fmaf(ysel[e], scc, shc) > 0.f ? pc * gout[e] : 0.f;
                row = arg[e];
            }
        }
    };
    fetch((long long)blockIdx.x * 4 + sub);
    for (long long g0 = (long long)blockIdx.x * 4; g0 < G; g0 += (long long)gridDim.x * 4) {
        const float cv = v;
        const int crow = row, cbase = base, cnrows = nrows;
        __syncthreads();                              // the previous round's rows are written (and Ws is there)
        mycf[c] = cv;
#pragma unroll
        for (int i = 0; i < MAXR * MW / 256; ++i) mymask[c + 256 * i] = 0u;
        __syncthreads();
        if (cv != 0.f && crow < cnrows) atomicOr(&mymask[crow * MW + (c >> 5)], 1u << (c & 31));
        __syncthreads();
        fetch(g0 + (long long)gridDim.x * 4 + sub);  // the next round's coefficients fly under this round's rows
        for (int r = rsub; r < cnrows; r += RPP) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            bool any = false;
#pragma unroll
            for (int w = 0; w < MW; ++w) {
                unsigned mm = mymask[r * MW + w];
                any = any || mm != 0u;
                while (mm) {
                    const int ch = 32 * w + __builtin_ctz(mm);
                    mm &= mm - 1u;
                    const float cw = mycf[ch];
                    const float4 wt = *reinterpret_cast<const float4 *>(&Ws[ch * KP + 4 * q]);
                    acc.x = fmaf(cw, wt.x, acc.x); acc.y = fmaf(cw, wt.y, acc.y);
                    acc.z = fmaf(cw, wt.z, acc.z); acc.w = fmaf(cw, wt.w, acc.w);
                }
            }
            const long long ri = (long long)cbase + r;
            if (any) *reinterpret_cast<float4 *>(&addend[ri * KP + 4 * q]) = acc;
            if (q == 0) rowmap[ri] = any ? (int)ri : -1;
        }
    }
}

// addend, software-pipelined (PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 1): a WAVE owns a group, so nothing of the walk crosses a wave
// and the loop holds no barrier at all (one __syncthreads behind the staging of W^T).  Lane l keeps the coefficient and the
// arg-max row of the channels l, l + 64, l + 128, l + 192 in registers; the channels that picked row r are then the ballots
// of (row == r), one 64-bit scalar per 64 channels, bit order = channel order -- no mask in LDS, no atomic, nothing to zero.
// The 64 lanes hold one row (KP / 64 floats each): the hit sequence is wave-uniform, so the bit scan, the loop control and the
// coefficient (v_readlane) are scalar work and a hit costs the vector pipe an address, a read and one fmaf (v_pk_fma at KP = 128).
// Pipeline: the first hit of each 64-channel word is a SLOT -- the four W^T reads of row r + 1 are issued (named register
// sets A / B, the loop written two rows per trip) before the fmaf of row r.  An empty word's bit scan gives -1: its slot
// reads the row in FRONT of the word's first channel (W^T is staged behind one spare row for word 0) and the coefficient of
// lane 63, without a select (scalar instructions issue once in four cycles per SIMD: they, not the vector pipe, set this
// kernel's pace), and its fmaf is skipped by a wave-uniform branch.  A word's second and later hits (256 channels spread
// over the group's rows: 0.6 per row at the SSG shape) follow in a plain loop.  Per row and column the fmaf chain is the
// former kernel's: the row's hits in ascending channel order from 0 -- the same bits.  The next group's (gout, ysel, arg)
// are requested before this group's rows, the block_start pair of the group after it one trip earlier.
template <int KP, int MAXR>
__global__ __launch_bounds__(1024) void pool_top_addend_rows_pipe_kernel(int G, int C, const float *__restrict__ gout,
                                                                         const float *__restrict__ ysel,
                                                                         const unsigned char *__restrict__ arg,
                                                                         const float *__restrict__ sc, const float *__restrict__ sh,
                                                                         const float *__restrict__ p, const float *__restrict__ Wt,
                                                                         const int *__restrict__ block_start,
                                                                         float *__restrict__ addend, int *__restrict__ rowmap) {
    constexpr int VEC = KP / 64, NW = 4;              // floats of a row per lane; 64-channel words (C <= 256)
    static_assert(VEC == 1 || VEC == 2, "a row is one or two floats per lane");
    static_assert(MAXR == 64 || MAXR == 128, "lane l answers for the rows l and l + 64 of a group");
    typedef float rowv_t __attribute__((ext_vector_type(VEC)));
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ws = lds + KP;                             // [C][KP] behind one spare row ("channel -1": read, never used)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the group index stays scalar
    for (int e = tid; e < C * (KP / 4); e += 1024)
        reinterpret_cast<float4 *>(Ws)[e] = reinterpret_cast<const float4 *>(Wt)[e];
    if (tid < KP) lds[tid] = 0.f;
    float scc[NW], shc[NW], pc[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int c = lane + 64 * k;
        scc[k] = c < C ? sc[c] : 0.f; shc[k] = c < C ? sh[c] : 0.f; pc[k] = c < C ? p[c] : 0.f;
    }
    __syncthreads();                                  // W^T is there; the only barrier
    // the group in flight: its raw triples (the coefficient is formed at use) and its rows
    float fy[NW], fg[NW];
    int fa[NW], fbase = 0, fn = 0;
    int nb0 = 0, nb1 = 0;                             // block_start pair of the group fetch() takes next (scalar loads)
    auto pair = [&](long long g) {
        if (g < G) { nb0 = block_start[g]; nb1 = block_start[g + 1]; }
    };
    auto fetch = [&](long long g) {
        fbase = 0; fn = 0;
        if (g < G) {
            fbase = kBlk * nb0;
            fn = kBlk * (nb1 - nb0);
            fn = fn < MAXR ? fn : MAXR;
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int c = lane + 64 * k;
            fy[k] = 0.f; fg[k] = 0.f; fa[k] = 0;
            if (g < G && c < C) {
                const long long e = g * C + c;
                fy[k] = ysel[e]; fg[k] = gout[e]; fa[k] = arg[e];
            }
        }
    };
    const long long stride = (long long)gridDim.x * 16;
    long long g = (long long)blockIdx.x * 16 + wave;
    // s_ff1_i32_b64: the lowest set bit, -1 for an empty word (__builtin_ctzll leaves that case undefined)
    auto ff1 = [](unsigned long long m) {
        int l;
        asm("s_ff1_i32_b64 %0, %1" : "=s"(l) : "s"(m));
        return l;
    };
    // one scalar instruction each (as C++ the mask is built with a 64-bit shift and, for the hit rows, kept in vector registers)
    auto bit_clear = [](unsigned long long &m, int l) { asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(l)); };
    auto bit_set = [](unsigned long long &m, int l) { asm("s_bitset1_b64 %0, %1" : "+s"(m) : "s"(l)); };
    // lane l's bytes of the row in front of word k's first channel: slot address = wbase[k] + (bit + 1) * KP * 4
    // (signed: word 0's base is -KP * 4 bytes from Ws, the spare row)
    int wbase[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) wbase[k] = ((64 * k - 1) * KP + VEC * lane) * 4;
    auto wrow = [&](int k, int l) {
        return *reinterpret_cast<const rowv_t *>(reinterpret_cast<const char *>(Ws) + (wbase[k] + (l + 1) * (KP * 4)));
    };
    pair(g);
    fetch(g);
    pair(g + stride);
    for (; g < G; g += stride) {
        int t0 = 0, t1 = 0;                           // the pair of the group after the next: requested here, waited for in
        if (g + 2 * stride < G) {                     // front of the row loop, whose lgkmcnt waits then count LDS reads only
            t0 = block_start[g + 2 * stride];
            t1 = block_start[g + 2 * stride + 1];
        }
        float cfv[NW];
        int rowv[NW];                                 // the row a channel adds to; -1: none (no coefficient, or beyond the group)
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            cfv[k] = fmaf(fy[k], scc[k], shc[k]) > 0.f ? pc[k] * fg[k] : 0.f;
            rowv[k] = (cfv[k] != 0.f && fa[k] < fn) ? fa[k] : -1;
        }
        const int base = fbase, nrows = fn;
        fetch(g + stride);                            // the next group's coefficients fly under this group's rows
        nb0 = t0; nb1 = t1;
        asm volatile("" ::"s"(nb0), "s"(nb1));
        // a register set: per word the hits, the first of them (-1: none), its W^T read and its coefficient
        struct Set {
            rowv_t w[NW];
            float cf[NW];
            unsigned long long m[NW];
            int l[NW];
        };
        auto coef = [&](int k, int l) {
            return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cfv[k]), l));
        };
        auto issue = [&](int r, Set &s) {
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                s.m[k] = __ballot(rowv[k] == r);
                s.l[k] = ff1(s.m[k]);
                s.cf[k] = coef(k, s.l[k]);
                s.w[k] = wrow(k, s.l[k]);
            }
        };
        unsigned long long anylo = 0ull, anyhi = 0ull; // the rows of the group with a hit (scalar)
        // the addend within a 32-bit byte offset: checked by the launcher
        char *const dst = reinterpret_cast<char *>(addend) + VEC * 4 * lane;
        auto finish = [&](int r, const Set &s) {
            rowv_t acc = 0.f;
            bool any = false;
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                if (s.l[k] >= 0) {
                    asm volatile("" ::: "memory");    // a branch, not a select: an empty slot costs the vector pipe nothing
                    any = true;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = fmaf(s.cf[k], s.w[k][i], acc[i]);
                    unsigned long long mm = s.m[k];
                    bit_clear(mm, s.l[k]);
                    while (mm) {
                        const int l = ff1(mm);
                        bit_clear(mm, l);
                        const float cw = coef(k, l);
                        const rowv_t wt = wrow(k, l);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(cw, wt[i], acc[i]);
                    }
                }
            }
            if (any) {
                *reinterpret_cast<rowv_t *>(dst + (unsigned)(base + r) * (unsigned)(KP * 4)) = acc;
                if (MAXR == 64 || r < 64) bit_set(anylo, r); else bit_set(anyhi, r - 64);
            }
        };
        Set A, B;
        issue(0, A);
        for (int r = 0; r < nrows; r += 2) {
            issue(r + 1, B);                          // a row beyond the group has no hit: dead channels carry row -1
            finish(r, A);
            issue(r + 2, A);
            if (r + 1 < nrows) finish(r + 1, B);
        }
        // rowmap [row] = row or -1 for every row of the group: lane l writes row l (and l + 64)
        if (lane < nrows) rowmap[(long long)base + lane] = (anylo >> lane) & 1ull ? base + lane : -1;
        if (MAXR > 64 && lane + 64 < nrows) rowmap[(long long)base + lane + 64] = (anyhi >> lane) & 1ull ? base + lane + 64 : -1;
    }
}

// wsparse: thread = channel, KP accumulators in registers; a workgroup walks its share of the groups, stages the group's
// rows of relu(bn(X)) (row stride KP + 1: the lanes of a wave read DIFFERENT rows at the same k -- conflict-free) and adds
// cf[g][c] X_g[arg][:].  part [gridDim.x][KP][C], part2 [gridDim.x][C]: summed in a fixed order by sum_partials2_kernel.
template <int KP>
__global__ __launch_bounds__(256) void pool_top_wsparse_rows_kernel(int G, int C, int maxr, const float *__restrict__ gout,
                                                                    const float *__restrict__ ysel,
                                                                    const unsigned char *__restrict__ arg,
                                                                    const float *__restrict__ sc, const float *__restrict__ sh,
                                                                    const float *__restrict__ p,
                                                                    const float *__restrict__ Yprev,
                                                                    const float *__restrict__ psc, const float *__restrict__ psh,
                                                                    const int *__restrict__ block_start,
                                                                    float *__restrict__ part, float *__restrict__ part2) {
    constexpr int LD = KP + 1, K4 = KP / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Xs = lds;                                  // [maxr][LD]
    const int tid = threadIdx.x, c = tid;             // C <= 256
    const float scc = c < C ? sc[c] : 0.f, shc = c < C ? sh[c] : 0.f, pc = c < C ? p[c] : 0.f;
    // a thread stages the column quad tid % K4 of the rows tid / K4, + 256 / K4, ...: its BN coefficients are fixed
    const int k4 = tid % K4, r0 = tid / K4;
    const float4 asc = *reinterpret_cast<const float4 *>(psc + 4 * k4), ash = *reinterpret_cast<const float4 *>(psh + 4 * k4);
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    float csum = 0.f;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const int b0 = block_start[g];
        int nrows = kBlk * (block_start[g + 1] - b0);
        nrows = nrows < maxr ? nrows : maxr;
        const float *src = Yprev + (long long)kBlk * b0 * KP;
        float cfv = 0.f;
        int row = 0;
        if (c < C) {
            const long long e = (long long)g * C + c;
            cfv = fmaf(ysel[e], scc, shc) > 0.f ? pc * gout[e] : 0.f;
            row = arg[e];
            if (row >= nrows) { row = 0; cfv = 0.f; }
        }
        __syncthreads();                              // the previous group's rows are consumed
        for (int r = r0; r < nrows; r += 256 / K4) {
            float4 x = *reinterpret_cast<const float4 *>(src + (long long)r * KP + 4 * k4);
            x.x = fmaxf(fmaf(x.x, asc.x, ash.x), 0.f); x.y = fmaxf(fmaf(x.y, asc.y, ash.y), 0.f);
            x.z = fmaxf(fmaf(x.z, asc.z, ash.z), 0.f); x.w = fmaxf(fmaf(x.w, asc.w, ash.w), 0.f);
            float *d = &Xs[r * LD + 4 * k4];
            d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        }
        __syncthreads();
        const float *xr = &Xs[row * LD];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] = fmaf(cfv, xr[k], acc[k]);
        csum += cfv;
    }
    if (c < C) {
        float *dst = part + (long long)blockIdx.x * KP * C + c;
#pragma unroll
        for (int k = 0; k < KP; ++k) dst[(long long)k * C] = acc[k];
        part2[(long long)blockIdx.x * C + c] = csum;
    }
}

// wsparse, software-pipelined (PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 1): the same thread = channel walk, but the NEXT group's rows
// (NR float4 per thread), its (gout, ysel, arg) triple and the block_start pair of the group after it are requested into
// registers before this group's accumulation, the LDS image is double-buffered (ONE barrier per group: a buffer is rewritten two
// groups later, behind the barrier that follows its last read), and a hit row is read with KP / 4 ds_read_b128 -- row stride
// KP + 4 floats = an odd number of 16-byte units, so the lanes of a read group that hold different rows mod 16 meet different
// units of the bank row (KP + 1 is the stride for ds_read_b32).  Same partition of the groups over the grid, same partial layout.
template <int KP, int NR>
__global__ __launch_bounds__(256) void pool_top_wsparse_rows_pipe_kernel(int G, int C, int maxr, const float *__restrict__ gout,
                                                                         const float *__restrict__ ysel,
                                                                         const unsigned char *__restrict__ arg,
                                                                         const float *__restrict__ sc, const float *__restrict__ sh,
                                                                         const float *__restrict__ p,
                                                                         const float *__restrict__ Yprev,
                                                                         const float *__restrict__ psc, const float *__restrict__ psh,
                                                                         const int *__restrict__ block_start,
                                                                         float *__restrict__ part, float *__restrict__ part2) {
    constexpr int LD = KP + 4, K4 = KP / 4, RPP = 256 / K4;       // rows staged per pass of the workgroup
    static_assert(NR * RPP == 64 || NR * RPP == 128, "the launcher sizes an LDS image at 64 or 128 rows (maxr <= NR RPP)");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, c = tid;                         // C <= 256
    const float scc = c < C ? sc[c] : 0.f, shc = c < C ? sh[c] : 0.f, pc = c < C ? p[c] : 0.f;
    const int k4 = tid % K4, r0 = tid / K4;
    const float4 asc = *reinterpret_cast<const float4 *>(psc + 4 * k4), ash = *reinterpret_cast<const float4 *>(psh + 4 * k4);
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    float csum = 0.f;
    const int grid = gridDim.x;
    // the group in flight: its rows, its raw triple (the coefficient is formed at use, not behind the load) and its row count
    float4 px[NR];
    float fy = 0.f, fg = 0.f;
    int fa = 0, fn = 0;
    int nb0 = 0, nb1 = 0;                                         // block_start pair of the group fetch() takes next
    auto pair = [&](int g) {
        if (g < G) { nb0 = block_start[g]; nb1 = block_start[g + 1]; }
    };
    // every request is unconditional: rows beyond the group's (and every row of a group beyond the last) lie outside the
    // buffer descriptor and read as zeros, the triple is read at a clamped index and dropped at use (fn == 0, c >= C)
    auto fetch = [&](int g) {
        const int n = g < G ? kBlk * (nb1 - nb0) : 0;
        fn = n < maxr ? n : maxr;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(Yprev + (long long)kBlk * (g < G ? nb0 : 0) * KP, (long long)fn * KP * 4);
#pragma unroll
        for (int j = 0; j < NR; ++j) px[j] = buf_load4(rx, (unsigned)((r0 + RPP * j) * KP + 4 * k4) * 4u, 0u);
        const long long e = (long long)(g < G ? g : G - 1) * C + (c < C ? c : C - 1);
        fy = ysel[e]; fg = gout[e]; fa = arg[e];
    };
    int g = blockIdx.x;
    pair(g);
    fetch(g);
    pair(g + grid);
    int buf = 0;
    for (; g < G; g += grid) {
        float *Xs = lds + buf * (NR * RPP * LD);                  // [NR RPP][LD]: a row beyond the group's arrives as zeros and is stored as relu(shift); never read (row < fn below)
        int t0 = 0, t1 = 0;                                       // block_start pair of the group after the next (scalar loads: requested
        if (g + 2 * grid < G) {                                   // here, so that the barrier below does not wait for them)
            t0 = block_start[g + 2 * grid];
            t1 = block_start[g + 2 * grid + 1];
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int r = r0 + RPP * j;
            float4 x = px[j];
            x.x = fmaxf(fmaf(x.x, asc.x, ash.x), 0.f); x.y = fmaxf(fmaf(x.y, asc.y, ash.y), 0.f);
            x.z = fmaxf(fmaf(x.z, asc.z, ash.z), 0.f); x.w = fmaxf(fmaf(x.w, asc.w, ash.w), 0.f);
            *reinterpret_cast<float4 *>(&Xs[r * LD + 4 * k4]) = x;
        }
        float cfv = fmaf(fy, scc, shc) > 0.f ? pc * fg : 0.f;
        int row = fa;
        if (row >= fn || c >= C) { row = 0; cfv = 0.f; }
        fetch(g + grid);                                          // the next group flies under this group's accumulation
        nb0 = t0; nb1 = t1;
        __syncthreads();
        const float *xr = &Xs[row * LD];
#pragma unroll
        for (int q = 0; q < K4; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(xr + 4 * q);
            acc[4 * q] = fmaf(cfv, v.x, acc[4 * q]); acc[4 * q + 1] = fmaf(cfv, v.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(cfv, v.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(cfv, v.w, acc[4 * q + 3]);
        }
        csum += cfv;
        buf ^= 1;
    }
    if (c < C) {
        float *dst = part + (long long)blockIdx.x * KP * C + c;
#pragma unroll
        for (int k = 0; k < KP; ++k) dst[(long long)k * C] = acc[k];
        part2[(long long)blockIdx.x * C + c] = csum;
    }
}

extern "C" {

/* compact arg-max rows of the data gradient: addend [(M/S) min(S,N)][Kp], rowmap [M] (slot or -1) */
int pcops_mlp_pool_top_addend(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                            const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                            const float *p, const float *Wt, float *addend, int *rowmap, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(M >= 1 && S >= 1 && S <= 256 && M % S == 0 && Kp % 4 == 0 && N >= 1 && N <= 65535);
    PCOPS_REQUIRE_PTR(gout); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax); PCOPS_REQUIRE_PTR(pool_scale);
    PCOPS_REQUIRE_PTR(pool_shift); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(Wt); PCOPS_REQUIRE_PTR(addend);
    PCOPS_REQUIRE_PTR(rowmap);
    if (reinterpret_cast<uintptr_t>(Wt) & 15 || reinterpret_cast<uintptr_t>(addend) & 15) return PCOPS_ERR_UNSUPPORTED;
    if (N > 1024 || Kp > 512) return PCOPS_ERR_UNSUPPORTED;
    if (M / S <= 512)
        hipLaunchKernelGGL(pool_top_addend_kernel<1024>, dim3(M / S), dim3(1024), 0, as_stream(stream), S, N, Kp,
                           S < N ? S : N, gout, ysel, argmax, pool_scale, pool_shift, p, Wt, addend, rowmap);
    else
        hipLaunchKernelGGL(pool_top_addend_kernel<256>, dim3(M / S), dim3(256), 0, as_stream(stream), S, N, Kp,
                           S < N ? S : N, gout, ysel, argmax, pool_scale, pool_shift, p, Wt, addend, rowmap);
    return pcops_launch_status();
}

/* Ssp [Kp][N] = X^T (p.G) (the arg-max rows only), cfsum [N] = column sums of p.G */
int pcops_mlp_pool_top_wsparse(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                               const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                               const float *p, const float *Yprev, const float *prev_scale, const float *prev_shift,
                               float *Ssp, float *cfsum, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(M >= 1 && S >= 1 && S <= 256 && M % S == 0 && Kp >= 1 && Kp <= 512 && N >= 1);
    PCOPS_REQUIRE_PTR(gout); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax); PCOPS_REQUIRE_PTR(pool_scale);
    PCOPS_REQUIRE_PTR(pool_shift); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(Yprev);
    PCOPS_REQUIRE_ARG((prev_scale == nullptr) == (prev_shift == nullptr));
    PCOPS_REQUIRE_PTR(Ssp); PCOPS_REQUIRE_PTR(cfsum);
    hipLaunchKernelGGL(pool_top_wsparse_kernel, dim3(N), dim3(256), 0, as_stream(stream), (long long)(M / S), S, N,
                       Kp, gout, ysel, argmax, pool_scale, pool_shift, p, Yprev, prev_scale, prev_shift, Ssp, cfsum);
    return pcops_launch_status();
}

/* ---- the four algebraic entry points over COMPACTED rows (pcops.h): rows == NULL is the entry point without the suffix */
unsigned long long pcops_mlp_pool_top_wsparse_rows_partial(int Kp, int N) {
    return (unsigned long long)kTopRowsWs * ((unsigned long long)Kp * N + N);
}

int pcops_mlp_pool_top_addend_rows(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                                   const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                                   const float *p, const float *Wt, float *addend, int *rowmap, const pcops_rows_t *rows,
                                   pcops_stream_t stream) {
    if (!rows) return pcops_mlp_pool_top_addend(M, Kp, N, S, gout, ysel, argmax, pool_scale, pool_shift, p, Wt, addend, rowmap, stream);
    PCOPS_REQUIRE_SHAPE(M >= 1 && S >= 1 && M % S == 0);
    PCOPS_REQUIRE_PTR(gout); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax); PCOPS_REQUIRE_PTR(pool_scale);
    PCOPS_REQUIRE_PTR(pool_shift); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(Wt); PCOPS_REQUIRE_PTR(addend);
    PCOPS_REQUIRE_PTR(rowmap);
    { const int rrc = rows_ok(rows); if (rrc) return rrc; }
    // this call's own share of pcops_mlp_pool_top_rows_supported: the floor on M there belongs to the Gram pass and the dense
    // products, the addend kernels take any number of groups
    if (!addend_rows_shape_ok(M, Kp, N, S)) return PCOPS_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(Wt) & 15 || reinterpret_cast<uintptr_t>(addend) & 15) return PCOPS_ERR_UNSUPPORTED;
    const int G = M / S;
    const size_t lds = ((size_t)N * Kp + 4 * 256 + 4 * 128 * 8) * sizeof(float);
    const int grid = (G + 3) / 4 < 256 ? (G + 3) / 4 : 256;
    hipStream_t st = as_stream(stream);
    // PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 1 (default): the wave-per-group kernel (both widths, S <= 64 and S <= 128; a wave takes
    // a group, 16 groups per workgroup and round).  Only W^T lives in LDS, behind one spare row.  Same rows, same rowmap, same bits.
    const bool piped = pcops_get_option(PCOPS_OPT_POOL_TOP_ROWS_PIPELINED) != 0;
    const size_t lds_pipe = (size_t)(N + 1) * Kp * sizeof(float);     // one spare row in front
    const int grid_pipe = (G + 15) / 16 < 256 ? (G + 15) / 16 : 256;
    return pcops_dispatch<64, 128>(Kp, PCOPS_ERR_UNSUPPORTED, [&](auto kp_) {
        constexpr int KP = decltype(kp_)::value;
        auto kern = !piped ? pool_top_addend_rows_kernel<KP>
                  : S <= 64 ? pool_top_addend_rows_pipe_kernel<KP, 64> : pool_top_addend_rows_pipe_kernel<KP, 128>;
        return pcops_launch_lds(kern, dim3(piped ? grid_pipe : grid), dim3(1024), piped ? lds_pipe : lds, 160 * 1024, st, G, N,
                                gout, ysel, argmax, pool_scale, pool_shift, p, Wt, rows->block_start, addend, rowmap);
    });
}

int pcops_mlp_pool_top_wsparse_rows(int M, int Kp, int N, int S, const float *gout, const float *ysel,
                                    const unsigned char *argmax, const float *pool_scale, const float *pool_shift,
                                    const float *p, const float *Yprev, const float *prev_scale, const float *prev_shift,
                                    float *Ssp, float *cfsum, float *partial, const pcops_rows_t *rows,
                                    pcops_stream_t stream) {
    if (!rows) return pcops_mlp_pool_top_wsparse(M, Kp, N, S, gout, ysel, argmax, pool_scale, pool_shift, p, Yprev, prev_scale, prev_shift, Ssp, cfsum, stream);
    PCOPS_REQUIRE_SHAPE(M >= 1 && S >= 1 && M % S == 0);
    PCOPS_REQUIRE_PTR(gout); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax); PCOPS_REQUIRE_PTR(pool_scale);
    PCOPS_REQUIRE_PTR(pool_shift); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(Yprev); PCOPS_REQUIRE_PTR(prev_scale);
    PCOPS_REQUIRE_PTR(prev_shift); PCOPS_REQUIRE_PTR(Ssp); PCOPS_REQUIRE_PTR(cfsum); PCOPS_REQUIRE_PTR(partial);
    { const int rrc = rows_ok(rows); if (rrc) return rrc; }
    if (!pcops_mlp_pool_top_rows_supported(M, Kp, N, S)) return PCOPS_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(Yprev) & 15 || reinterpret_cast<uintptr_t>(prev_scale) & 15 ||
        reinterpret_cast<uintptr_t>(prev_shift) & 15)
        return PCOPS_ERR_UNSUPPORTED;
    const int G = M / S;
    const int grid = G < kTopRowsWs ? G : kTopRowsWs;
    const size_t lds = (size_t)S * (Kp + 1) * sizeof(float);
    float *part2 = partial + (long long)kTopRowsWs * Kp * N;
    hipStream_t st = as_stream(stream);
    // PCOPS_OPT_POOL_TOP_ROWS_PIPELINED = 1 (default): the software-pipelined kernel (both widths; NR = the float4 a thread
    // holds of a group of S rows).  Same grid, so pcops_mlp_pool_top_wsparse_rows_partial covers both.
    // two images of NR x (256 / (Kp / 4)) = 64 or 128 rows each: every row a group can have, because
    // pcops_mlp_pool_top_rows_supported (checked above) caps S at 128
    const int img_rows = S <= 64 ? 64 : 128;
    if (S > img_rows) return PCOPS_ERR_UNSUPPORTED;
    const size_t lds_pipe = (size_t)2 * img_rows * (Kp + 4) * sizeof(float);
    const bool piped = pcops_get_option(PCOPS_OPT_POOL_TOP_ROWS_PIPELINED) != 0;
    const int rc = pcops_dispatch<64, 128>(Kp, PCOPS_ERR_UNSUPPORTED, [&](auto kp_) {
        constexpr int KP = decltype(kp_)::value;
        auto kern = !piped ? pool_top_wsparse_rows_kernel<KP>
                  : S <= 64 ? pool_top_wsparse_rows_pipe_kernel<KP, KP / 16> : pool_top_wsparse_rows_pipe_kernel<KP, KP / 8>;
        return pcops_launch_lds(kern, dim3(grid), dim3(256), piped ? lds_pipe : lds, 160 * 1024, st, G, N, S, gout, ysel, argmax,
                                pool_scale, pool_shift, p, Yprev, prev_scale, prev_shift, rows->block_start, partial, part2);
    });
    if (rc) return rc;
    const long long L = (long long)Kp * N;
    return pcops_mlp_sum_partials2(grid, L, partial, Ssp, (long long)N, part2, cfsum, st);
}

int pcops_mlp_dy_apply(long long M, int N, const float *G, const float *Y, const float *p, const float *q, const float *t,
                       float *out, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(M >= 0 && N >= 4 && N % 4 == 0);
    if (M == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(G); PCOPS_REQUIRE_PTR(Y); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(q); PCOPS_REQUIRE_PTR(t); PCOPS_REQUIRE_PTR(out);
    PCOPS_REQUIRE_ARG(((uintptr_t)G | (uintptr_t)Y | (uintptr_t)p | (uintptr_t)q | (uintptr_t)t | (uintptr_t)out) % 16 == 0);
    const long long total4 = M * (N / 4);
    const unsigned grid = (unsigned)(cdiv(total4, 256) < 8192 ? cdiv(total4, 256) : 8192);
    hipLaunchKernelGGL(dy_apply_kernel, dim3(grid), dim3(256), 0, as_stream(stream), total4, N / 4,
                       reinterpret_cast<const float4 *>(G), reinterpret_cast<const float4 *>(Y),
                       reinterpret_cast<const float4 *>(p), reinterpret_cast<const float4 *>(q),
                       reinterpret_cast<const float4 *>(t), reinterpret_cast<float4 *>(out));
    return pcops_launch_status();
}

int pcops_mlp_pool_top_prep(int Kp, int N, const float *W, const float *b, const float *q, const float *t, float *Wt,
                            float *Wq, float *u, float *v, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(Kp >= 1 && N >= 1);
    PCOPS_REQUIRE_PTR(W); PCOPS_REQUIRE_PTR(b); PCOPS_REQUIRE_PTR(q); PCOPS_REQUIRE_PTR(t);
    PCOPS_REQUIRE_PTR(Wt); PCOPS_REQUIRE_PTR(Wq); PCOPS_REQUIRE_PTR(u);
    const int gx = (N + 31) / 32;
    hipLaunchKernelGGL(pool_top_prep_kernel, dim3(gx, (Kp + 31) / 32 + (v ? ((Kp + 7) / 8 + gx - 1) / gx : 0)), dim3(256), 0,
                       as_stream(stream), Kp, N, W, b, q, t, Wt, Wq, u, v);
    return pcops_launch_status();
}

int pcops_mlp_pool_top_finish(int Kp, int N, long long M, float *dW, const float *Ssp, const float *xsum, const float *u,
                              const float *cfsum, const float *q, const float *W, const float *b, const float *t,
                              float *db, pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(Kp >= 1 && N >= 1 && M >= 1);
    PCOPS_REQUIRE_PTR(dW); PCOPS_REQUIRE_PTR(Ssp); PCOPS_REQUIRE_PTR(xsum); PCOPS_REQUIRE_PTR(u); PCOPS_REQUIRE_PTR(cfsum);
    PCOPS_REQUIRE_PTR(q); PCOPS_REQUIRE_PTR(W); PCOPS_REQUIRE_PTR(b); PCOPS_REQUIRE_PTR(t); PCOPS_REQUIRE_PTR(db);
    hipLaunchKernelGGL(pool_top_finish_kernel, dim3((N + 255) / 256, 8 + (Kp + 7) / 8), dim3(256), 0, as_stream(stream), Kp, N,
                       (float)M, dW, Ssp, xsum, u, cfsum, q, W, b, t, db);
    return pcops_launch_status();
}

}  // extern "C"
