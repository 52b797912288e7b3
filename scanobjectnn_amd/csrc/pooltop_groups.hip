// pooltop_groups.hip -- the algebraic backward of a pooled top layer over UNCOMPACTED rows in small groups (pcops.h
// "algebraic backward of a pooled top layer", the *_groups entry points): 64 -> N, S = 32 / 64, millions of rows.
//
//   dX = mask . (X Mq + v + (p.G) W^T)              Mq = W diag(q) W^T, v = W (q.b + t)
//   dW = (X^T X) Wq + (X^T 1) u^T + X^T (p.G)       db = 1^T (p.G) + ...        (closed by pcops_mlp_pool_top_finish)
//
// With S = 32 and N = 128 nearly every row is some channel's arg-max, so the compact addend of pcops_mlp_pool_top_addend
// would be as large as X.  Here the sparse halves never leave the chip: two kernels, each ONE pass over Yprev,
//   dgrad_top_groups_kernel   X Mq on the fp32 matrix pipe (Mq resident in registers), a tile's addend rows built from
//                             (gout, ysel, argmax) and the LDS-resident W^T, epilogue + statistics, one float4 store
//   dgrad_top_groups_mm_kernel   the same at N = 128 with the tile's addend as ONE product P W^T on split bf16 operands, the
//                             default there (PCOPS_POOL_TOP_GROUPS_MM=0: the kernel above for every N)
//   wgrad_top_groups_kernel   X^T X (upper 32 x 32 blocks), X^T 1, X^T (p.G), 1^T (p.G) from one staged image of X
// Both are persistent over 64-row tiles (whole groups), the next tile's rows and (gout, ysel, argmax) triples requested
// before this tile's arithmetic.  No float atomics; every sum in a fixed order (channel-ascending per row, tiles in
// ascending order per workgroup, partial copies in index order): two runs give the same bits.
#include "common.h"

namespace {

constexpr int KP = 64;            // input width of the layer (the only one these kernels are built for)
constexpr int TR = 64;            // rows per tile: two groups of 32 or one of 64
constexpr int XLD = KP + 4;       // row stride of a staged tile in floats: 16-byte reads of whole rows without bank conflicts
constexpr int NMAX = 256;         // widest layer
constexpr int MW = NMAX / 32;     // mask words per row
constexpr int kMaxGrid = 512;

// what a thread holds of a tile between its request and its use: its four float4 of Yprev and the (group, channel) triples
// tid, tid + 256.  The float4 i of a thread sits at (trow, tcol): ROWS = false, 16 rows of 16 threads four times (the weight
// gradient); ROWS = true, one row per four threads, the row's 64-byte quarters dealt round (the data gradient, whose addend
// walk and epilogue own whole rows)
struct TileRegs {
    float4 y[4];
    float go[2], ys[2];
    int am[2];
};
template <bool ROWS> __device__ __forceinline__ int trow(int i) { return ROWS ? (int)(threadIdx.x >> 2) : 16 * i + (int)(threadIdx.x >> 4); }
template <bool ROWS> __device__ __forceinline__ int tcol(int i) { return ROWS ? 4 * ((int)(threadIdx.x & 3) + 4 * i) : 4 * (int)(threadIdx.x & 15); }

template <bool ROWS>
__device__ __forceinline__ void tile_request(TileRegs &t, long long tile, long long ntiles, long long M, long long G, int N,
                                             int gpt, const float *__restrict__ Yprev, const float *__restrict__ gout,
                                             const float *__restrict__ ysel, const unsigned char *__restrict__ arg) {
    // every load is unconditional at a clamped address (a request past the end re-reads the last row / group and is never
    // used): a guarded load would be waited for where the guard merges, and the request would not run ahead of the tile
    const int tid = threadIdx.x;
    const long long tl = tile < ntiles ? tile : ntiles - 1;
    // (the triples first: what is done to them on arrival then waits for them alone, not for the rows behind them)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int e = tid + 256 * j;                 // (group in tile, channel) = (e / N, e % N)
        const int gl = e / N;
        const long long g = tl * gpt + (gl < gpt ? gl : 0);
        const long long o = (g < G ? g : G - 1) * N + (e - gl * N);
        t.go[j] = gout[o]; t.ys[j] = ysel[o]; t.am[j] = arg[o];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = tl * TR + trow<ROWS>(i);
        t.y[i] = *reinterpret_cast<const float4 *>(Yprev + (r < M ? r : M - 1) * KP + tcol<ROWS>(i));
    }
}

// cf of the triple j of this thread (pool_top_addend's coefficient): p g where relu(bn(ysel)) > 0; 0 for a triple past the end.
// pv = pool_scale, pool_shift, p [NMAX] each, IN LDS: a global load here would be waited for with vmcnt(0), behind the
// request of the next tile
__device__ __forceinline__ float triple_cf(const TileRegs &t, int j, long long tile, long long G, int N, int gpt,
                                           const float *pv) {
    const int e = threadIdx.x + 256 * j, gl = e / N, c = e - gl * N;
    if (gl >= gpt || tile * gpt + gl >= G) return 0.f;
    return fmaf(t.ys[j], pv[c], pv[NMAX + c]) > 0.f ? pv[2 * NMAX + c] * t.go[j] : 0.f;
}

__device__ __forceinline__ float4 bn_relu4(float4 y, float4 sc, float4 sh, bool in) {
    float4 x;
    x.x = in ? fmaxf(fmaf(y.x, sc.x, sh.x), 0.f) : 0.f;
    x.y = in ? fmaxf(fmaf(y.y, sc.y, sh.y), 0.f) : 0.f;
    x.z = in ? fmaxf(fmaf(y.z, sc.z, sh.z), 0.f) : 0.f;
    x.w = in ? fmaxf(fmaf(y.w, sc.w, sh.w), 0.f) : 0.f;
    return x;
}

// ------------------------------------------------------------------------------------------------ data gradient
// 256 threads.  Product: wave w owns the 32 x 32 block (w >> 1, w & 1) of the tile's 64 x 64 result.  Staging, addend walk
// and epilogue: thread = (row tid / 4, the row's quarters tid % 4 + 4 k), so the raw Yprev a thread loaded and the addend it
// built stay in its registers until the store.  LDS: W^T [N][WLD], the staged X tile, the product tile, the per-channel
// vectors, cf [gpt][N], the per-row channel masks.  Two barriers per tile.
constexpr int WLD = KP + 4;

__global__ __launch_bounds__(256) void dgrad_top_groups_kernel(long long M, int N, int S, const float *__restrict__ Yprev,
                                                               const float *__restrict__ psc, const float *__restrict__ psh,
                                                               const float *__restrict__ Mq, const float *__restrict__ vconst,
                                                               const float *__restrict__ gout, const float *__restrict__ ysel,
                                                               const unsigned char *__restrict__ arg,
                                                               const float *__restrict__ sc, const float *__restrict__ sh,
                                                               const float *__restrict__ p, const float *__restrict__ Wt,
                                                               float *__restrict__ Gprev, float *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *wts = lds;                                 // [N][WLD]
    float *xs = wts + N * WLD;                        // [TR][XLD]
    float *os = xs + TR * XLD;                        // [TR][XLD]
    float *cst = os + TR * XLD;                       // prev_scale, prev_shift, vconst [KP] each
    float *cfl = cst + 3 * KP;                        // [2][NMAX]
    float *pv = cfl + 2 * NMAX;                       // pool_scale, pool_shift, p [NMAX] each
    unsigned *mask = reinterpret_cast<unsigned *>(pv + 3 * NMAX);       // [TR][MW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = tid >> 2, qj = tid & 3;
    const int gpt = TR / S, nw2 = (N + 63) / 64;
    const long long G = M / S, ntiles = (M + TR - 1) / TR;

    for (int i = tid; i < N * KP / 4; i += 256)
        *reinterpret_cast<float4 *>(wts + (i >> 4) * WLD + 4 * (i & 15)) = reinterpret_cast<const float4 *>(Wt)[i];
    for (int i = tid; i < TR * MW; i += 256) mask[i] = 0u;
    if (tid < KP) { cst[tid] = psc[tid]; cst[KP + tid] = psh[tid]; cst[2 * KP + tid] = vconst[tid]; }
    if (tid < N) { pv[tid] = sc[tid]; pv[NMAX + tid] = sh[tid]; pv[2 * NMAX + tid] = p[tid]; }
    // the wave's 32 columns of Mq as the B operand: step (j, e) multiplies k = 8 j + 4 h + e (h = lane / 32)
    const int l32 = lane & 31, h = lane >> 5, row0 = 32 * (wave >> 1), col0 = 32 * (wave & 1);
    float bq[32];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) bq[4 * j + e] = Mq[(8 * j + 4 * h + e) * KP + col0 + l32];
    float4 s1[4], s2[4];                              // sum dX, sum dX Yprev of this thread's row slot
#pragma unroll
    for (int k = 0; k < 4; ++k) s1[k] = s2[k] = make_float4(0.f, 0.f, 0.f, 0.f);

    const float *cfg = cfl + (row / S) * NMAX;
    const float *wrow = wts + 4 * qj;
    unsigned long long *mrow = reinterpret_cast<unsigned long long *>(mask + row * MW);
    // one tile: `cur` holds its rows and triples, the next tile's are requested into `nxt`.  The loop below calls it with
    // the two register sets swapped instead of copying one into the other: a copy would wait for the request (and for this
    // tile's stores) at the end of every tile
    auto do_tile = [&](long long tile, TileRegs &cur, TileRegs &nxt) {
        tile_request<true>(nxt, tile + gridDim.x, ntiles, M, G, N, gpt, Yprev, gout, ysel, arg);
        const bool in = tile * TR + row < M;
        // ---- stage X = relu(bn(Yprev)) (rows past the end: zero), the coefficients and the per-row channel masks
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = tcol<true>(k);
            *reinterpret_cast<float4 *>(xs + row * XLD + c) =
                bn_relu4(cur.y[k], *reinterpret_cast<const float4 *>(cst + c), *reinterpret_cast<const float4 *>(cst + KP + c), in);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = tid + 256 * j, gl = e / N, c = e - gl * N;
            if (gl < gpt) {
                const float cf = triple_cf(cur, j, tile, G, N, gpt, pv);
                cfl[gl * NMAX + c] = cf;
                if (cf != 0.f && cur.am[j] < S) atomicOr(&mask[(gl * S + cur.am[j]) * MW + (c >> 5)], 1u << (c & 31));
            }
        }
        __syncthreads();
        // ---- X Mq: 32 steps of the 32 x 32 x 2 fp32 MFMA, A read as whole float4
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 a = *reinterpret_cast<const float4 *>(xs + (row0 + l32) * XLD + 8 * j + 4 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq[4 * j + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq[4 * j + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq[4 * j + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq[4 * j + 3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            os[(row0 + 8 * (i >> 2) + 4 * h + (i & 3)) * XLD + col0 + l32] = acc[i];
        // ---- the addend of this thread's row: the channels that picked it in ascending order, 64 mask bits at a time, the
        // next channel's W^T quarters requested before this one's are used; the mask is cleared behind
        float4 add[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) add[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int w2 = 0; w2 < nw2; ++w2) {
            unsigned long long m = mrow[w2];
            if (qj == 0) mrow[w2] = 0ull;
            int c = m ? 64 * w2 + __builtin_ctzll(m) : 0;
            float cfn = m ? cfg[c] : 0.f;
            float4 wn[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) wn[k] = *reinterpret_cast<const float4 *>(wrow + c * WLD + 16 * k);
            while (m) {
                m &= m - 1;
                const float cf = cfn;
                float4 wc[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wc[k] = wn[k];
                c = m ? 64 * w2 + __builtin_ctzll(m) : 0;
                cfn = m ? cfg[c] : 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) wn[k] = *reinterpret_cast<const float4 *>(wrow + c * WLD + 16 * k);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    add[k].x = fmaf(cf, wc[k].x, add[k].x); add[k].y = fmaf(cf, wc[k].y, add[k].y);
                    add[k].z = fmaf(cf, wc[k].z, add[k].z); add[k].w = fmaf(cf, wc[k].w, add[k].w);
                }
            }
        }
        __syncthreads();
        // ---- epilogue: (acc + v) + addend under the ReLU mask of X, statistics, the row's quarters stored as float4
        if (in) {
            float *dst = Gprev + (tile * TR + row) * KP;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = tcol<true>(k);
                const float4 o = *reinterpret_cast<const float4 *>(os + row * XLD + c);
                const float4 vsc = *reinterpret_cast<const float4 *>(cst + c), vsh = *reinterpret_cast<const float4 *>(cst + KP + c);
                const float4 vc = *reinterpret_cast<const float4 *>(cst + 2 * KP + c);
                const float4 y = cur.y[k];
                float4 d;
                d.x = fmaf(y.x, vsc.x, vsh.x) > 0.f ? (o.x + vc.x) + add[k].x : 0.f;
                d.y = fmaf(y.y, vsc.y, vsh.y) > 0.f ? (o.y + vc.y) + add[k].y : 0.f;
                d.z = fmaf(y.z, vsc.z, vsh.z) > 0.f ? (o.z + vc.z) + add[k].z : 0.f;
                d.w = fmaf(y.w, vsc.w, vsh.w) > 0.f ? (o.w + vc.w) + add[k].w : 0.f;
                *reinterpret_cast<float4 *>(dst + c) = d;
                s1[k].x += d.x; s1[k].y += d.y; s1[k].z += d.z; s1[k].w += d.w;
                s2[k].x = fmaf(d.x, y.x, s2[k].x); s2[k].y = fmaf(d.y, y.y, s2[k].y);
                s2[k].z = fmaf(d.z, y.z, s2[k].z); s2[k].w = fmaf(d.w, y.w, s2[k].w);
            }
        }
    };
    TileRegs ra, rb;
    tile_request<true>(ra, blockIdx.x, ntiles, M, G, N, gpt, Yprev, gout, ysel, arg);
    __syncthreads();
    for (long long tile = blockIdx.x; tile < ntiles; tile += 2 * gridDim.x) {
        do_tile(tile, ra, rb);
        if (tile + gridDim.x < ntiles) do_tile(tile + gridDim.x, rb, ra);
    }
    // ---- the workgroup's statistics row: the 64 row slots of a column added in index order
    __syncthreads();
    float *red = xs;                                  // [TR][2][KP], over the two tiles
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        *reinterpret_cast<float4 *>(red + (row * 2 + 0) * KP + tcol<true>(k)) = s1[k];
        *reinterpret_cast<float4 *>(red + (row * 2 + 1) * KP + tcol<true>(k)) = s2[k];
    }
    __syncthreads();
    if (tid < 2 * KP) {
        float s = 0.f;
        for (int i = 0; i < TR; ++i) s += red[i * 2 * KP + tid];
        stats[(long long)blockIdx.x * 2 * KP + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------ data gradient, N = 128
// The same tile loop with the tile's addend as ONE product on the 16-bit matrix pipe: addend = P W^T, P [64][N] with
// P[r][c] = cf[g(r)][c] where argmax[g(r)][c] == r, else 0.  Its cost is fixed -- it does not depend on how the hits are spread
// over the rows -- where the walk above is serial in a row's hits.  Split operands (device.h split3_pair: x = h + m + l in bf16
// pieces), six products hh | lh, mh, mm, hm, hl on v_mfma_f32_32x32x16_bf16, large and small terms in separate accumulators.
//   B  W^T's pieces as ready fragments in LDS, split once per workgroup: [piece][k-step][column block][lane] x 8 bf16 (48 KB)
//   A  built in registers: the triple owners store cf pre-split (three bf16 arrays) and the arg-max bytes per (group, channel);
//      for a k-step a lane at (row, half) reads 8 arg-max bytes and 3 x 8 pieces (one address per half: broadcast reads) and
//      keeps the entries whose arg-max is its row.  An arg-max >= S equals no row; cf == 0 is three zero pieces.
// X Mq runs on split operands as well (24 instead of 32 matrix instructions of twice the length; measured).
// The wave that owns a 32 x 32 block holds X Mq and the addend in the same accumulator layout and writes (acc + v) + addend
// into the tile image that held X (one more barrier; a thread's epilogue reads exactly the floats its next staging overwrites).
// LDS 78.5 KB: two workgroups per CU.  N = 128 is the only width <= 128 the *_groups forms take (N >= 2 Kp).
constexpr int NM = 128;           // the width of the matrix form
constexpr int NKS = NM / 16;      // its k-steps

// Four arg-max bytes XORed with the lane's row (every byte < 128: the staged arg-max is clamped to 127, a row is < 64) -> 0xff
// in the bytes that are zero, four bytes at a time: (x | 0x80) - 1 keeps bit 7 of a byte unless the byte was zero and never
// borrows from its neighbour.  The pair of words that mask a fragment's four bf16 pairs is the mask's bytes doubled (v_perm).
// (As a compare and a select per byte the fragment build was 56 of a k-step's 70 vector instructions.)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) {
    const unsigned hit = ~((x | 0x80808080u) - 0x01010101u) & 0x80808080u;
    return (hit << 1) - (hit >> 7);
}
__device__ __forceinline__ unsigned double_bytes(unsigned m, int hi) {
    return __builtin_amdgcn_perm(m, m, hi ? 0x03030202u : 0x01010000u);
}

__global__ __launch_bounds__(256, 2) void dgrad_top_groups_mm_kernel(int M, int S, const float *__restrict__ Yprev,
                                                                     const float *__restrict__ psc, const float *__restrict__ psh,
                                                                     const float *__restrict__ Mq, const float *__restrict__ vconst,
                                                                     const float *__restrict__ gout, const float *__restrict__ ysel,
                                                                     const unsigned char *__restrict__ arg,
                                                                     const float *__restrict__ sc, const float *__restrict__ sh,
                                                                     const float *__restrict__ p, const float *__restrict__ Wt,
                                                                     float *__restrict__ Gprev, float *__restrict__ stats) {
    constexpr int N = NM;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4 *wf = reinterpret_cast<u32x4 *>(lds);                              // [3][NKS][2][64] fragments of 8 bf16
    float *xs = lds + 3 * NKS * 2 * 64 * 4;                                  // [TR][XLD]: X, then the result tile
    float *cst = xs + TR * XLD;                                              // prev_scale, prev_shift, vconst [KP] each
    float *pv = cst + 3 * KP;                                                // pool_scale, pool_shift, p [NMAX] each
    unsigned short *cfp = reinterpret_cast<unsigned short *>(pv + 3 * NMAX);  // [3 pieces][2 groups][NM]
    unsigned char *amb = reinterpret_cast<unsigned char *>(cfp + 3 * 2 * NM);  // [2 groups][NM]
    u32x4 *qlf = reinterpret_cast<u32x4 *>(amb + 2 * NM);                     // Mq's third piece, [4 k-steps][2][64] fragments
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = tid >> 2;
    const int gpt = TR / S;
    const int G = M / S, ntiles = (M + TR - 1) / TR;

    // W^T [N][KP] as B fragments: element j of lane (l32, h) at k-step ks, column block cb is W^T[16 ks + 8 h + j][32 cb + l32]
    for (int i = tid; i < NKS * 2 * 64; i += 256) {
        const float *src = Wt + (16 * (i >> 7) + 8 * ((i >> 5) & 1)) * KP + 32 * ((i >> 6) & 1) + (i & 31);
        u32x4 fh, fm, fl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned a, b, c;
            split3_pair(src[2 * q * KP], src[(2 * q + 1) * KP], a, b, c);
            fh[q] = a; fm[q] = b; fl[q] = c;
        }
        wf[i] = fh; wf[NKS * 128 + i] = fm; wf[2 * NKS * 128 + i] = fl;
    }
    if (tid < KP) { cst[tid] = psc[tid]; cst[KP + tid] = psh[tid]; cst[2 * KP + tid] = vconst[tid]; }
    if (tid < N) { pv[tid] = sc[tid]; pv[NMAX + tid] = sh[tid]; pv[2 * NMAX + tid] = p[tid]; }
    const int l32 = lane & 31, h = lane >> 5, row0 = 32 * (wave >> 1), col0 = 32 * (wave & 1);
    // the wave's 32 columns of Mq as the B operand, three bf16 pieces: element j of k-step ks is Mq[16 ks + 8 h + j][col0 + l32].
    // The two large pieces in registers, the third in LDS (with all three in registers hipcc spilled 20 bytes a lane)
    u32x4 qh[4], qm[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float *src = Mq + (16 * ks + 8 * h + 2 * q) * KP + col0 + l32;
            unsigned a, b, c;
            split3_pair(src[0], src[KP], a, b, c);
            qh[ks][q] = a; qm[ks][q] = b;
            if (wave < 2) reinterpret_cast<unsigned *>(qlf + (2 * ks + wave) * 64 + lane)[q] = c;
        }
    float4 s1[4], s2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s1[k] = s2[k] = make_float4(0.f, 0.f, 0.f, 0.f);

    // the wave's rows lie in ONE group: group (S = 32: its row block; S = 64: the tile's only one) and the lane's row in it
    const int glw = S == 32 ? (wave >> 1) : 0;
    const unsigned rig4 = (unsigned)((S == 32 ? 0 : row0) + l32) * 0x01010101u;
    const unsigned short *cfa = cfp + glw * NM + 8 * h;
    const unsigned char *ama = amb + glw * NM + 8 * h;
    const u32x4 *wfa = wf + 64 * (wave & 1) + lane;
    // the request and the triple in 32-bit indices (M Kp 4 < 2^31: groups_shape_ok; as 64-bit values the group count lived in
    // a register pair that hipcc spilled, and a scratch reload in the tile body is a vector-memory load waited for with
    // vmcnt(0) behind the request).  One triple per thread: gpt N <= 256.  Unconditional loads at clamped addresses, as above.
    const int gch = tid & (NM - 1), ggl = tid >> 7;                           // the thread's (group in tile, channel)
    auto request = [&](TileRegs &t, int tile) {
        const int tl = tile < ntiles ? tile : ntiles - 1;
        const int g = tl * gpt + (ggl < gpt ? ggl : 0);
        const unsigned o = (unsigned)(g < G ? g : G - 1) * NM + gch;
        t.go[0] = gout[o]; t.ys[0] = ysel[o]; t.am[0] = arg[o];
        const int r = tl * TR + row;
        const float *src = Yprev + (unsigned)(r < M ? r : M - 1) * KP;
#pragma unroll
        for (int i = 0; i < 4; ++i) t.y[i] = *reinterpret_cast<const float4 *>(src + tcol<true>(i));
    };
    auto do_tile = [&](int tile, TileRegs &cur, TileRegs &nxt) {
        request(nxt, tile + (int)gridDim.x);
        const bool in = tile * TR + row < M;
        // ---- stage X = relu(bn(Yprev)) (rows past the end: zero), the coefficients' pieces and the arg-max bytes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = tcol<true>(k);
            *reinterpret_cast<float4 *>(xs + row * XLD + c) =
                bn_relu4(cur.y[k], *reinterpret_cast<const float4 *>(cst + c), *reinterpret_cast<const float4 *>(cst + KP + c), in);
        }
        if (tid < gpt * N) {
            // cf (pool_top_addend's coefficient): p g where relu(bn(ysel)) > 0; 0 for a group past the end
            const bool live = tile * gpt + ggl < G && fmaf(cur.ys[0], pv[gch], pv[NMAX + gch]) > 0.f;
            unsigned ch, cm, cl;
            split3_pair(live ? pv[2 * NMAX + gch] * cur.go[0] : 0.f, 0.f, ch, cm, cl);
            cfp[tid] = (unsigned short)ch; cfp[2 * NM + tid] = (unsigned short)cm; cfp[4 * NM + tid] = (unsigned short)cl;
            amb[tid] = (unsigned char)(cur.am[0] < 127 ? cur.am[0] : 127);   // (>= S either way: it equals no row)
        }
        __syncthreads();
        // ---- X Mq on split operands too: four k-steps, X's pieces made from the staged fp32 row as it is read
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, accs = acc;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float *xr = xs + (row0 + l32) * XLD + 16 * ks + 8 * h;
            const float4 x0 = *reinterpret_cast<const float4 *>(xr), x1 = *reinterpret_cast<const float4 *>(xr + 4);
            u32x4 xh, xm, xl;
            { unsigned a, b, c; split3_pair(x0.x, x0.y, a, b, c); xh[0] = a; xm[0] = b; xl[0] = c; }
            { unsigned a, b, c; split3_pair(x0.z, x0.w, a, b, c); xh[1] = a; xm[1] = b; xl[1] = c; }
            { unsigned a, b, c; split3_pair(x1.x, x1.y, a, b, c); xh[2] = a; xm[2] = b; xl[2] = c; }
            { unsigned a, b, c; split3_pair(x1.z, x1.w, a, b, c); xh[3] = a; xm[3] = b; xl[3] = c; }
            const bf16x8 ah = __builtin_bit_cast(bf16x8, xh), am = __builtin_bit_cast(bf16x8, xm), al = __builtin_bit_cast(bf16x8, xl);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, qh[ks]), bm = __builtin_bit_cast(bf16x8, qm[ks]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, qlf[(2 * ks + (wave & 1)) * 64 + lane]);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, accs, 0, 0, 0);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, accs, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, accs, 0, 0, 0);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, accs, 0, 0, 0);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, accs, 0, 0, 0);
        }
        acc += accs;
        // ---- the addend of the wave's block, P W^T over ascending channel blocks of 16
        f32x16 big = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sml = big;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const uint2 a = *reinterpret_cast<const uint2 *>(ama + 16 * ks);
            u32x4 ph = *reinterpret_cast<const u32x4 *>(cfa + 16 * ks);
            u32x4 pm = *reinterpret_cast<const u32x4 *>(cfa + 2 * NM + 16 * ks);
            u32x4 pl = *reinterpret_cast<const u32x4 *>(cfa + 4 * NM + 16 * ks);
            const unsigned m0 = zero_bytes(a.x ^ rig4), m1 = zero_bytes(a.y ^ rig4);
            const u32x4 mk = {double_bytes(m0, 0), double_bytes(m0, 1), double_bytes(m1, 0), double_bytes(m1, 1)};
            ph &= mk; pm &= mk; pl &= mk;
            const bf16x8 ah = __builtin_bit_cast(bf16x8, ph), am = __builtin_bit_cast(bf16x8, pm), al = __builtin_bit_cast(bf16x8, pl);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, wfa[ks * 128]);
            const bf16x8 bm = __builtin_bit_cast(bf16x8, wfa[(NKS + ks) * 128]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, wfa[(2 * NKS + ks) * 128]);
            sml = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, sml, 0, 0, 0);
            sml = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, sml, 0, 0, 0);
            big = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, big, 0, 0, 0);
            sml = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, sml, 0, 0, 0);
            sml = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, sml, 0, 0, 0);
            sml = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, sml, 0, 0, 0);
        }
        __syncthreads();                                                     // every wave has read X
        const float vc = cst[2 * KP + col0 + l32];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            xs[(row0 + 8 * (i >> 2) + 4 * h + (i & 3)) * XLD + col0 + l32] = (acc[i] + vc) + (big[i] + sml[i]);
        __syncthreads();
        // ---- epilogue: the ReLU mask of X, statistics, the row's quarters stored as float4
        if (in) {
            float *dst = Gprev + (unsigned)(tile * TR + row) * KP;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = tcol<true>(k);
                const float4 o = *reinterpret_cast<const float4 *>(xs + row * XLD + c);
                const float4 vsc = *reinterpret_cast<const float4 *>(cst + c), vsh = *reinterpret_cast<const float4 *>(cst + KP + c);
                const float4 y = cur.y[k];
                float4 d;
                d.x = fmaf(y.x, vsc.x, vsh.x) > 0.f ? o.x : 0.f;
                d.y = fmaf(y.y, vsc.y, vsh.y) > 0.f ? o.y : 0.f;
                d.z = fmaf(y.z, vsc.z, vsh.z) > 0.f ? o.z : 0.f;
                d.w = fmaf(y.w, vsc.w, vsh.w) > 0.f ? o.w : 0.f;
                *reinterpret_cast<float4 *>(dst + c) = d;
                s1[k].x += d.x; s1[k].y += d.y; s1[k].z += d.z; s1[k].w += d.w;
                s2[k].x = fmaf(d.x, y.x, s2[k].x); s2[k].y = fmaf(d.y, y.y, s2[k].y);
                s2[k].z = fmaf(d.z, y.z, s2[k].z); s2[k].w = fmaf(d.w, y.w, s2[k].w);
            }
        }
    };
    TileRegs ra, rb;
    request(ra, (int)blockIdx.x);
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += 2 * (int)gridDim.x) {
        do_tile(tile, ra, rb);
        if (tile + (int)gridDim.x < ntiles) do_tile(tile + (int)gridDim.x, rb, ra);
    }
    // ---- the workgroup's statistics row: the 64 row slots of a column added in index order
    __syncthreads();
    float *red = lds;                                // [TR][2][KP], over the fragments of W^T
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        *reinterpret_cast<float4 *>(red + (row * 2 + 0) * KP + tcol<true>(k)) = s1[k];
        *reinterpret_cast<float4 *>(red + (row * 2 + 1) * KP + tcol<true>(k)) = s2[k];
    }
    __syncthreads();
    if (tid < 2 * KP) {
        float s = 0.f;
        for (int i = 0; i < TR; ++i) s += red[i * 2 * KP + tid];
        stats[(long long)blockIdx.x * 2 * KP + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// 256 threads.  Dense half: wave w multiplies rows 16 w .. 16 w + 15 of the tile into the three upper 32 x 32 blocks of
// X^T X (48 accumulators, carried over every tile of the workgroup).  Sparse half: thread = (channel, k part); a group's
// arg-max row of the staged image read with 16-byte LDS reads, KP / KS accumulators.  KS = 2 for N <= 128 (every thread
// busy), 1 above.  The partial copy of a workgroup: gram [KP][KP] (mirrored), xsum [KP], Ssp [KP][N], cfsum [N].
template <int KS>
__global__ __launch_bounds__(256) void wgrad_top_groups_kernel(long long M, int N, int S, const float *__restrict__ Yprev,
                                                               const float *__restrict__ psc, const float *__restrict__ psh,
                                                               const float *__restrict__ gout, const float *__restrict__ ysel,
                                                               const unsigned char *__restrict__ arg,
                                                               const float *__restrict__ sc, const float *__restrict__ sh,
                                                               const float *__restrict__ p, float *__restrict__ partial) {
    constexpr int KW = KP / KS;                       // columns of X a sparse thread accumulates
    __shared__ __attribute__((aligned(16))) float xs[TR * XLD];
    __shared__ float cfl[2 * NMAX];
    __shared__ int aml[2 * NMAX];
    __shared__ float pv[3 * NMAX];                    // pool_scale, pool_shift, p
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rr = tid >> 4, q = tid & 15;
    const int gpt = TR / S;
    const long long G = M / S, ntiles = (M + TR - 1) / TR;
    const int l32 = lane & 31, h = lane >> 5;
    const int cch = KS == 2 ? (tid & 127) : tid, k0 = KS == 2 ? 32 * (tid >> 7) : 0;      // sparse half: channel, first column
    const float4 vsc = *reinterpret_cast<const float4 *>(psc + 4 * q), vsh = *reinterpret_cast<const float4 *>(psh + 4 * q);

    f32x16 g00 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, g01 = g00, g11 = g00;
    float4 xsum = make_float4(0.f, 0.f, 0.f, 0.f);
    float sp[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) sp[k] = 0.f;
    float cfs = 0.f;

    if (tid < N) { pv[tid] = sc[tid]; pv[NMAX + tid] = sh[tid]; pv[2 * NMAX + tid] = p[tid]; }
    __syncthreads();
    TileRegs cur, nxt;
    tile_request<false>(cur, blockIdx.x, ntiles, M, G, N, gpt, Yprev, gout, ysel, arg);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        tile_request<false>(nxt, tile + gridDim.x, ntiles, M, G, N, gpt, Yprev, gout, ysel, arg);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 x = bn_relu4(cur.y[i], vsc, vsh, tile * TR + 16 * i + rr < M);
            *reinterpret_cast<float4 *>(xs + (16 * i + rr) * XLD + 4 * q) = x;
            xsum.x += x.x; xsum.y += x.y; xsum.z += x.z; xsum.w += x.w;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = tid + 256 * j, gl = e / N, c = e - gl * N;
            if (gl < gpt) {
                cfl[gl * NMAX + c] = triple_cf(cur, j, tile, G, N, gpt, pv);
                aml[gl * NMAX + c] = cur.am[j] < S ? cur.am[j] : S - 1;
            }
        }
        __syncthreads();
        // ---- X^T X: the wave's 16 rows are its k range, 8 steps x 3 blocks
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const float *xr = xs + (16 * wave + 2 * st + h) * XLD;
            const float f0 = xr[l32], f1 = xr[32 + l32];
            g00 = __builtin_amdgcn_mfma_f32_32x32x2f32(f0, f0, g00, 0, 0, 0);
            g01 = __builtin_amdgcn_mfma_f32_32x32x2f32(f0, f1, g01, 0, 0, 0);
            g11 = __builtin_amdgcn_mfma_f32_32x32x2f32(f1, f1, g11, 0, 0, 0);
        }
        // ---- X^T (p.G): the groups of the tile in ascending order
        // (a thread past the last channel adds zeros of row 0: no branch between the MFMA chain and these reads)
        for (int gl = 0; gl < gpt; ++gl) {
            const float cf = cch < N ? cfl[gl * NMAX + cch] : 0.f;
            const float *xr = xs + (gl * S + (cch < N ? aml[gl * NMAX + cch] : 0)) * XLD + k0;
#pragma unroll
            for (int k = 0; k < KW; k += 4) {
                const float4 x = *reinterpret_cast<const float4 *>(xr + k);
                sp[k + 0] = fmaf(cf, x.x, sp[k + 0]); sp[k + 1] = fmaf(cf, x.y, sp[k + 1]);
                sp[k + 2] = fmaf(cf, x.z, sp[k + 2]); sp[k + 3] = fmaf(cf, x.w, sp[k + 3]);
            }
            cfs += cf;
        }
        __syncthreads();
        cur = nxt;
    }
    // ---- the workgroup's partial copy
    float *part = partial + (long long)blockIdx.x * (KP * KP + KP + KP * N + N);
    float *pg = part, *px = pg + KP * KP, *ps = px + KP, *pc = ps + KP * N;
    // Gram blocks: the four waves' accumulators added in wave order through LDS (3 x 1024 floats), then written mirrored
    float *red = xs;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int o = (8 * (i >> 2) + 4 * h + (i & 3)) * 32 + l32;
                if (w == 0) { red[o] = g00[i]; red[1024 + o] = g01[i]; red[2048 + o] = g11[i]; }
                else { red[o] += g00[i]; red[1024 + o] += g01[i]; red[2048 + o] += g11[i]; }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < KP * KP; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int br = r >> 5, bc = c >> 5;
        float v;
        if (br <= bc) v = red[(br + bc) * 1024 + (r & 31) * 32 + (c & 31)];
        else v = red[1024 + (c & 31) * 32 + (r & 31)];
        pg[i] = v;
    }
    __syncthreads();
    // xsum: the 16 row slots of a column quarter in index order
    *reinterpret_cast<float4 *>(red + rr * KP + 4 * q) = xsum;
    __syncthreads();
    if (tid < KP) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += red[i * KP + tid];
        px[tid] = s;
    }
    if (cch < N) {
#pragma unroll
        for (int k = 0; k < KW; ++k) ps[(k0 + k) * N + cch] = sp[k];
        if (k0 == 0) pc[cch] = cfs;
    }
}

// out[i] = the P partial copies of element i added in a fixed order (16 lanes of copies, then the lanes in index order);
// the copy is [L] floats with the four outputs behind one another
__global__ __launch_bounds__(1024) void groups_sum_kernel(int P, int L, int N, const float *__restrict__ part,
                                                          float *__restrict__ gram, float *__restrict__ xsum,
                                                          float *__restrict__ Ssp, float *__restrict__ cfsum) {
    __shared__ double sm[16][64];
    const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + c;
    double s = 0.0;
    if (i < L)
        for (int pp = pl; pp < P; pp += 16) s += (double)part[(long long)pp * L + i];
    sm[pl][c] = s;
    __syncthreads();
    if (pl == 0 && i < L) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sm[k][c];
        const int o1 = KP * KP, o2 = o1 + KP, o3 = o2 + KP * N;
        float *dst = i < o1 ? gram + i : i < o2 ? xsum + (i - o1) : i < o3 ? Ssp + (i - o2) : cfsum + (i - o3);
        *dst = (float)t;
    }
}

// what the kernels themselves take (the planner's answer adds a floor on M)
bool groups_shape_ok(long long M, int Kp, int N, int S) {
    return Kp == KP && N % 32 == 0 && N >= 64 && N <= NMAX && N >= 2 * Kp && (S == 32 || S == 64) && M >= S && M % S == 0 &&
           M * Kp * 4 < (long long)kOOB;
}

int groups_grid(long long M) {
    const long long ntiles = (M + TR - 1) / TR;
    return (int)(ntiles < kMaxGrid ? ntiles : kMaxGrid);
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

}  // namespace

extern "C" {

int pcops_mlp_stats_rows(int M);

// Below 262 144 rows Y (M N 4 bytes at N = 128) is at most half of the 256 MB cache level and the store this form removes
// is not an HBM store (reasoned, not measured); no stored launch trace reaches 131 072 rows at this shape.
int pcops_mlp_pool_top_groups_supported(int M, int Kp, int N, int S) {
    return groups_shape_ok(M, Kp, N, S) && M >= 262144 ? 1 : 0;
}

int pcops_mlp_pool_top_groups_partial(int M, int Kp, int N) {
    if (M < 1 || Kp != KP || N < 1 || N > NMAX) return 0;
    return groups_grid(M) * (Kp * Kp + Kp + Kp * N + N);
}

int pcops_mlp_dgrad_top_groups(int M, int Kp, int N, int S, const float *Yprev, const float *prev_scale,
                               const float *prev_shift, const float *Mq, const float *vconst, const float *gout,
                               const float *ysel, const unsigned char *argmax, const float *pool_scale,
                               const float *pool_shift, const float *p, const float *Wt, float *Gprev, float *stats_partial,
                               pcops_stream_t stream) {
    if (!groups_shape_ok(M, Kp, N, S)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(Yprev); PCOPS_REQUIRE_PTR(prev_scale); PCOPS_REQUIRE_PTR(prev_shift); PCOPS_REQUIRE_PTR(Mq);
    PCOPS_REQUIRE_PTR(vconst); PCOPS_REQUIRE_PTR(gout); PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax);
    PCOPS_REQUIRE_PTR(pool_scale); PCOPS_REQUIRE_PTR(pool_shift); PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(Wt);
    PCOPS_REQUIRE_PTR(Gprev); PCOPS_REQUIRE_PTR(stats_partial);
    if (!aligned16(Yprev) || !aligned16(prev_scale) || !aligned16(prev_shift) || !aligned16(vconst) || !aligned16(Wt) ||
        !aligned16(Gprev))
        return PCOPS_ERR_UNSUPPORTED;
    // one workgroup per statistics row: pcops_mlp_stats_rows(M) never exceeds the 64-row tiles nor kMaxGrid
    const int grid = pcops_mlp_stats_rows(M);
    if (grid < 1 || grid > kMaxGrid || grid > (M + TR - 1) / TR) return PCOPS_ERR_UNSUPPORTED;
    // PCOPS_POOL_TOP_GROUPS_MM = 1 (default): N = 128 takes the addend as a product on the 16-bit matrix pipe; 0: the walk
    static const bool mm_on = pcops_env_switch("PCOPS_POOL_TOP_GROUPS_MM", true);   // kernel A/B only
    if (mm_on && N == NM) {
        const size_t lds = (size_t)(3 * NKS * 2 * 64 * 4 + TR * XLD + 3 * KP + 3 * NMAX) * sizeof(float) + 3 * 2 * NM * 2 + 2 * NM +
                           4 * 2 * 64 * 16;
        pcops_note_pipe(1);
        return pcops_launch_lds(dgrad_top_groups_mm_kernel, dim3(grid), dim3(256), lds, 160 * 1024, as_stream(stream), M, S, Yprev,
                                prev_scale, prev_shift, Mq, vconst, gout, ysel, argmax, pool_scale, pool_shift, p, Wt, Gprev,
                                stats_partial);
    }
    const size_t lds = (size_t)(N * WLD + 2 * TR * XLD + 3 * KP + 5 * NMAX + TR * MW) * sizeof(float);
    pcops_note_pipe(0);
    return pcops_launch_lds(dgrad_top_groups_kernel, dim3(grid), dim3(256), lds, 160 * 1024, as_stream(stream), (long long)M, N,
                            S, Yprev, prev_scale, prev_shift, Mq, vconst, gout, ysel, argmax, pool_scale, pool_shift, p, Wt,
                            Gprev, stats_partial);
}

int pcops_mlp_wgrad_top_groups(int M, int Kp, int N, int S, const float *Yprev, const float *prev_scale,
                               const float *prev_shift, const float *gout, const float *ysel, const unsigned char *argmax,
                               const float *pool_scale, const float *pool_shift, const float *p, float *partial, float *gram,
                               float *xsum, float *Ssp, float *cfsum, pcops_stream_t stream) {
    if (!groups_shape_ok(M, Kp, N, S)) return PCOPS_ERR_UNSUPPORTED;
    PCOPS_REQUIRE_PTR(Yprev); PCOPS_REQUIRE_PTR(prev_scale); PCOPS_REQUIRE_PTR(prev_shift); PCOPS_REQUIRE_PTR(gout);
    PCOPS_REQUIRE_PTR(ysel); PCOPS_REQUIRE_PTR(argmax); PCOPS_REQUIRE_PTR(pool_scale); PCOPS_REQUIRE_PTR(pool_shift);
    PCOPS_REQUIRE_PTR(p); PCOPS_REQUIRE_PTR(partial); PCOPS_REQUIRE_PTR(gram); PCOPS_REQUIRE_PTR(xsum); PCOPS_REQUIRE_PTR(Ssp);
    PCOPS_REQUIRE_PTR(cfsum);
    if (!aligned16(Yprev) || !aligned16(prev_scale) || !aligned16(prev_shift)) return PCOPS_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const int grid = groups_grid(M), L = Kp * Kp + Kp + Kp * N + N;
    pcops_note_pipe(0);
    if (N <= 128)
        hipLaunchKernelGGL(wgrad_top_groups_kernel<2>, dim3(grid), dim3(256), 0, st, (long long)M, N, S, Yprev, prev_scale,
                           prev_shift, gout, ysel, argmax, pool_scale, pool_shift, p, partial);
    else
        hipLaunchKernelGGL(wgrad_top_groups_kernel<1>, dim3(grid), dim3(256), 0, st, (long long)M, N, S, Yprev, prev_scale,
                           prev_shift, gout, ysel, argmax, pool_scale, pool_shift, p, partial);
    hipLaunchKernelGGL(groups_sum_kernel, dim3(cdiv(L, 64)), dim3(1024), 0, st, grid, L, N, partial, gram, xsum, Ssp, cfsum);
    return pcops_launch_status();
}

}  // extern "C"
