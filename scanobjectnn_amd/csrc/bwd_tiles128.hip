// bwd_tiles128.hip -- the one-pass backward of a 128 -> 128 layer  Y = relu(bn(Yprev)) W + b  whose input rows are read (SA2's
// middle layer), with or without compacted rows: pcops_mlp_bwd_tiles_rows.
//
//   X  = max(fmaf(Yprev, a_scale, a_shift), 0),  m = fmaf(Yprev, a_scale, a_shift) > 0
//   dY = fmaf(p, G, w fmaf(q, Y, t))             w = the block's weight on a row that opens a 16-row block of a compacted set, else 1
//   dW = X^T dY,  db = 1^T dY,  Gprev = m . (dY W^T),  stats = (sum Gprev, sum Gprev Yprev) per column
//
// what pcops_mlp_gemm_dgrad_rows (with Yprev) followed by pcops_mlp_wgrad_rows compute, with every tensor read once.  The recipe is
// xyz_bwd_tiles.hip's; what differs is the budget: W^T's three pieces are 96 KB, so they live in REGISTERS.
//   * persistent workgroups of 512 threads, tiles of 32 rows dealt in ascending order; all eight waves take part in every tile
//   * wave w owns Gprev columns 16 w .. 16 w + 15: its slice of W^T (128 x 16 x 3 pieces) is 48 VGPRs of B fragments of
//     v_mfma_f32_16x16x32_bf16, loaded and split once.  It owns 16 rows of dW as well (8 blocks, 32 accumulators carried over
//     every tile; the small products of a tile are summed apart and join once per tile)
//   * STAGE: G and Y in row layout (thread = column quad cq, row pair rg), Yprev in STRIP layout (wave w reads columns 16 w ..,
//     lane = row pair m, quad qd) -- so the raw Yprev a lane needs for the mask and the statistics of ITS wave's Gprev block is
//     already in its registers and the epilogue is wave-local.  Requests are unconditional buffer loads with 32-bit offsets,
//     two tiles ahead; rows past the device row count are outside the descriptor and read as zeros.
//     dY is formed once, split into three bf16 pieces once and stored twice: row-major R (A operand of dX) and transposed T
//     (B operand of dW); X's pieces are stored transposed only (A operand of dW).  Column c of either T image lives in slot
//     32 (c % 4) + c / 4; 16-byte units are XORed with bits of the row / slot (conflict-free fragment reads without padding)
//   * two LDS images: a tile is computed from one while the next is staged into the other, ONE barrier per tile.  Waves 0..3 stage
//     first and compute second, waves 4..7 the other way round: a SIMD holds one wave of each, so one's vector / LDS-store work
//     runs under the other's matrix chain
//   * the Gprev block of a wave goes through a wave-private 1 KB LDS strip per 16 rows into the strip layout: mask, statistics,
//     16-byte stores
// No float atomics; every sum has a fixed order: two calls give the same bits.
#include "common.h"

namespace {

constexpr int KC = 128;                        // K == N == 128
constexpr int TR = 32;                         // rows of a tile
constexpr int PIECE = TR * KC * 2;             // bytes of one piece of an image (8 192)
constexpr int IMG = 9 * PIECE;                 // R, T (dY), TX (X): 73 728 bytes per tile image
constexpr int E_OFF = 2 * IMG;                 // the waves' strips [8][16 rows][16 floats]
constexpr int CO_OFF = E_OFF + 8 * 1024;       // p, q, t, a_scale, a_shift [128] each
constexpr int LDS_BYTES = CO_OFF + 5 * KC * 4; // 158 208

struct RowBlock { int g, s0; float w; int pad; };   // pcops_rows_t.blocks (pcops.h)
// a block record at a wave-uniform index through the constant address space: one scalar load (mlp.hip has the reasoning)
__device__ __forceinline__ float block_weight(const RowBlock *table, int i) {
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) i32x4_ *kptr;
    const i32x4_ v = *(kptr)(table + i);
    return __int_as_float(v.z);
}


struct Req {
    float4 g[2], y[2], x[2];       // two rows of G and Y (row layout), two rows of Yprev (strip layout)
    float w0, w1;                  // weights of the tile's two blocks
};

__device__ __forceinline__ void keep4(float4 &d, const float4 &v) {
    asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                 : "=&v"(d.x), "=&v"(d.y), "=&v"(d.z), "=&v"(d.w) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
}

// the unit swizzle of a T image: slot s
__device__ __forceinline__ int tswz(int s) { return (((s >> 1) ^ (s >> 3)) & 1) | (((s >> 2) & 1) << 1); }

template <bool ROWS, bool NT>
__global__ __launch_bounds__(512, 1) void bwd_tiles128_kernel(int Mall, const int *__restrict__ Mdev, const RowBlock *__restrict__ blocks,
                                                              const float *__restrict__ Yprev, const float *__restrict__ asc,
                                                              const float *__restrict__ ash, const float *__restrict__ G,
                                                              const float *__restrict__ Y, const float *__restrict__ p,
                                                              const float *__restrict__ q, const float *__restrict__ t,
                                                              const float *__restrict__ W, float *__restrict__ part,
                                                              float *__restrict__ dbpart, float *__restrict__ Gprev,
                                                              float *__restrict__ gstats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, nn = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hf = wave >> 2;
    // row layout: cq = column quad, rg = row pair (a 32-lane half is 8 quads x 4 row pairs: the T stores spread over all banks)
    const int cq = 8 * ((tid >> 5) & 3) + (tid & 7), rg = 4 * (tid >> 7) + ((tid >> 3) & 3);
    // strip layout: row pair m, quad qd of the wave's 16 columns
    const int m = lane >> 2, qd = lane & 3;
    int M = Mall;
    if (ROWS) {
        M = *Mdev;
        M = M < 0 ? 0 : (M > Mall ? Mall : M);
    }
    const int ntiles = (M + TR - 1) / TR, nblk = (M + 15) / 16;
    const int grp = blockIdx.x, ngrp = gridDim.x;
    const int cnt = grp < ntiles ? (ntiles - grp + ngrp - 1) / ngrp : 0;         // tiles of this workgroup

    float *co = reinterpret_cast<float *>(lds + CO_OFF);
    unsigned char *Es = lds + E_OFF + wave * 1024;
    if (tid < KC) {
        co[tid] = p[tid]; co[KC + tid] = q[tid]; co[2 * KC + tid] = t[tid];
        co[3 * KC + tid] = asc[tid]; co[4 * KC + tid] = ash[tid];
    }
    // ---- once: the wave's slice of W^T as B fragments -- element j of lane (nn, g4) at k-step ks is W[16 w + nn][32 ks + 8 g4 + j]
    u32x4 wh[4], wm[4], wl[4];
    {
        const float *src = W + (16 * wave + nn) * KC + 8 * g4;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 f0 = *reinterpret_cast<const float4 *>(src + 32 * ks), f1 = *reinterpret_cast<const float4 *>(src + 32 * ks + 4);
            const float wv[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
            split3_frag(wv, wh[ks], wm[ks], wl[ks]);
        }
    }
    __syncthreads();

    f32x4 accw[8];                                                              // dW rows (slots) 16 w .., column slots 16 nb ..
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) accw[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};            // of columns 16 w + 4 qd ..

    // ---- addresses that do not change
    // T (dY): slot 32 e + cq, rows 2 rg, 2 rg + 1 = word rg % 4 of unit rg / 4
    const int twr = cq * 64 + (((rg >> 2) ^ tswz(cq)) << 4) + 4 * (rg & 3);      // + e * 2048 (32 e leaves the swizzle as it is)
    // R: row r, columns 4 cq .. = half cq % 2 of unit cq / 2 at unit ^ (r % 16)
    const int r0 = 2 * rg;
    const int rw0 = r0 * 256 + (((cq >> 1) ^ (r0 & 15)) << 4) + 8 * (cq & 1);
    const int rw1 = (r0 + 1) * 256 + (((cq >> 1) ^ ((r0 + 1) & 15)) << 4) + 8 * (cq & 1);
    // TX: slot 32 e + 4 w + qd, rows 2 m, 2 m + 1
    const int xs = 4 * wave + qd;
    const int xwr = xs * 64 + (((m >> 2) ^ tswz(xs)) << 4) + 4 * (m & 3);
    // fragment reads: dX's A operand = R row 16 rbk + nn, unit 4 ks + g4;  dW's operands = slot 16 b + nn, unit g4
    const int ard = nn * 256;
    const int trd = nn * 64;

    const __amdgpu_buffer_rsrc_t rG = make_rsrc_u32(G, (unsigned)M * (KC * 4u)), rY = make_rsrc_u32(Y, (unsigned)M * (KC * 4u)),
                                 rX = make_rsrc_u32(Yprev, (unsigned)M * (KC * 4u)),
                                 rO = make_rsrc_u32(Gprev, (unsigned)M * (KC * 4u));
    const unsigned gvo = (unsigned)(2 * rg * KC + 4 * cq) * 4u, xvo = (unsigned)(2 * m * KC + 16 * wave + 4 * qd) * 4u;
    auto request = [&](Req &r, int tile) {
        tile = tile < ntiles ? tile : ntiles - 1;
        tile = tile < 0 ? 0 : tile;
        const unsigned so = (unsigned)tile * (TR * KC * 4u);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            r.g[j] = buf_load4(rG, gvo + j * KC * 4u, so);
            r.y[j] = buf_load4(rY, gvo + j * KC * 4u, so);
            r.x[j] = buf_load4(rX, xvo + j * KC * 4u, so);
        }
        r.w0 = r.w1 = 1.f;
        if (ROWS) {
            int b0 = 2 * tile, b1 = b0 + 1;
            b0 = b0 < nblk ? b0 : nblk - 1; b0 = b0 < 0 ? 0 : b0;
            b1 = b1 < nblk ? b1 : nblk - 1; b1 = b1 < 0 ? 0 : b1;
            r.w0 = block_weight(blocks, b0);
            r.w1 = block_weight(blocks, b1);
        }
    };

    // a row past M is a zero row of dY: an exact zero in every sum (its X is finite: its Yprev reads as zeros)
    auto stage = [&](const Req &r, int tile, unsigned char *img) {
        unsigned char *Rb = img, *Tb = img + 3 * PIECE, *Xb = img + 6 * PIECE;
        const int row0 = tile * TR;
        {   // ---- dY
            const float4 cp = *reinterpret_cast<const float4 *>(co + 4 * cq), cqv = *reinterpret_cast<const float4 *>(co + KC + 4 * cq),
                         ct = *reinterpret_cast<const float4 *>(co + 2 * KC + 4 * cq);
            // the row that opens a block: rows 0 and 16 of the tile
            const float w = ROWS ? (rg == 0 ? r.w0 : (rg == 8 ? r.w1 : 1.f)) : 1.f;
            float d[2][4];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 g = r.g[j], y = r.y[j];
                d[j][0] = fmaf(cp.x, g.x, (ROWS && j == 0) ? w * fmaf(cqv.x, y.x, ct.x) : fmaf(cqv.x, y.x, ct.x));
                d[j][1] = fmaf(cp.y, g.y, (ROWS && j == 0) ? w * fmaf(cqv.y, y.y, ct.y) : fmaf(cqv.y, y.y, ct.y));
                d[j][2] = fmaf(cp.z, g.z, (ROWS && j == 0) ? w * fmaf(cqv.z, y.z, ct.z) : fmaf(cqv.z, y.z, ct.z));
                d[j][3] = fmaf(cp.w, g.w, (ROWS && j == 0) ? w * fmaf(cqv.w, y.w, ct.w) : fmaf(cqv.w, y.w, ct.w));
                if (!(row0 + r0 + j < M)) d[j][0] = d[j][1] = d[j][2] = d[j][3] = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) dbs[e] += d[j][e];
            }
            unsigned ph[4], pm[4], pl[4];                                        // [column]: rows r0 (low half), r0 + 1
#pragma unroll
            for (int e = 0; e < 4; ++e) split3_pair(d[0][e], d[1][e], ph[e], pm[e], pl[e]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned char *dst = Tb + twr + e * 2048;
                *reinterpret_cast<unsigned *>(dst) = ph[e];
                *reinterpret_cast<unsigned *>(dst + PIECE) = pm[e];
                *reinterpret_cast<unsigned *>(dst + 2 * PIECE) = pl[e];
            }
            auto lo = [](unsigned a, unsigned b) { return (a & 0xffffu) | (b << 16); };
            auto hi = [](unsigned a, unsigned b) { return (a >> 16) | (b & 0xffff0000u); };
            *reinterpret_cast<u32x2 *>(Rb + rw0) = u32x2{lo(ph[0], ph[1]), lo(ph[2], ph[3])};
            *reinterpret_cast<u32x2 *>(Rb + rw0 + PIECE) = u32x2{lo(pm[0], pm[1]), lo(pm[2], pm[3])};
            *reinterpret_cast<u32x2 *>(Rb + rw0 + 2 * PIECE) = u32x2{lo(pl[0], pl[1]), lo(pl[2], pl[3])};
            *reinterpret_cast<u32x2 *>(Rb + rw1) = u32x2{hi(ph[0], ph[1]), hi(ph[2], ph[3])};
            *reinterpret_cast<u32x2 *>(Rb + rw1 + PIECE) = u32x2{hi(pm[0], pm[1]), hi(pm[2], pm[3])};
            *reinterpret_cast<u32x2 *>(Rb + rw1 + 2 * PIECE) = u32x2{hi(pl[0], pl[1]), hi(pl[2], pl[3])};
        }
        {   // ---- X (a row past M is finite and meets a zero row of dY)
            const float4 sc = *reinterpret_cast<const float4 *>(co + 3 * KC + 16 * wave + 4 * qd),
                         sh = *reinterpret_cast<const float4 *>(co + 4 * KC + 16 * wave + 4 * qd);
            float x[2][4];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 v = r.x[j];
                x[j][0] = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f);
                x[j][1] = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
                x[j][2] = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f);
                x[j][3] = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned a, b, c;
                split3_pair(x[0][e], x[1][e], a, b, c);
                unsigned char *dst = Xb + xwr + e * 2048;
                *reinterpret_cast<unsigned *>(dst) = a;
                *reinterpret_cast<unsigned *>(dst + PIECE) = b;
                *reinterpret_cast<unsigned *>(dst + 2 * PIECE) = c;
            }
        }
    };
    // yk: the raw Yprev of the tile in the strip layout (kept from its request)
    auto compute = [&](int tile, const unsigned char *img, const float4 (&yk)[2]) {
        const unsigned char *Rb = img, *Tb = img + 3 * PIECE, *Xb = img + 6 * PIECE;
        // ---- dX blocks [16 rows][16 columns] x 2 = dY W^T: 4 k-steps x 2 row blocks x 6 products
        f32x4 accd[2], smd[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) accd[b] = smd[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 ah[2], am[2], al[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const unsigned char *src = Rb + (16 * b) * 256 + ard + (((4 * ks + g4) ^ nn) << 4);
                ah[b] = frag(*reinterpret_cast<const u32x4 *>(src));
                am[b] = frag(*reinterpret_cast<const u32x4 *>(src + PIECE));
                al[b] = frag(*reinterpret_cast<const u32x4 *>(src + 2 * PIECE));
            }
            const bf16x8 bh = frag(wh[ks]), bm = frag(wm[ks]), bl = frag(wl[ks]);
#define PCOPS_BT_MM(A_, B_, C_)                                                                     \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                   \
        C_[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A_[b], B_, C_[b], 0, 0, 0)
            PCOPS_BT_MM(al, bh, smd);
            PCOPS_BT_MM(ah, bh, accd);
            PCOPS_BT_MM(am, bm, smd);
            PCOPS_BT_MM(am, bh, smd);
            PCOPS_BT_MM(ah, bl, smd);
            PCOPS_BT_MM(ah, bm, smd);
#undef PCOPS_BT_MM
            __builtin_amdgcn_sched_barrier(0);
        }
        accd[0] += smd[0]; accd[1] += smd[1];

        // ---- Gprev: each 16-row block through the wave's strip into the strip layout (ahead of the dW product: its stores have
        // that product's time to leave before the next staging waits on the request behind them)
        const float4 sc = *reinterpret_cast<const float4 *>(co + 3 * KC + 16 * wave + 4 * qd),
                     sh = *reinterpret_cast<const float4 *>(co + 4 * KC + 16 * wave + 4 * qd);
        const unsigned so = (unsigned)tile * (TR * KC * 4u);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 4; ++r)      // row 4 g4 + r, column nn: quad nn / 4 at (nn / 4) ^ g4
                *reinterpret_cast<float *>(Es + (4 * g4 + r) * 64 + (((nn >> 2) ^ g4) << 4) + 4 * (nn & 3)) = accd[b][r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // branch-free (the lanes of the other block add zeros and store past the descriptor): the stores of a tile are a
            // fixed count, so the wait in front of the next staging is a vmcnt(n) on the request, not a vmcnt(0) on them
            const bool mine = (m >> 3) == b;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int rl = 2 * (m & 7) + j;
                float4 o = *reinterpret_cast<const float4 *>(Es + rl * 64 + ((qd ^ ((rl >> 2) & 3)) << 4));
                const float4 yp = yk[j];
                o.x = (mine && fmaf(yp.x, sc.x, sh.x) > 0.f) ? o.x : 0.f;
                o.y = (mine && fmaf(yp.y, sc.y, sh.y) > 0.f) ? o.y : 0.f;
                o.z = (mine && fmaf(yp.z, sc.z, sh.z) > 0.f) ? o.z : 0.f;
                o.w = (mine && fmaf(yp.w, sc.w, sh.w) > 0.f) ? o.w : 0.f;
                s1[0] += o.x; s1[1] += o.y; s1[2] += o.z; s1[3] += o.w;
                s2[0] = fmaf(o.x, yp.x, s2[0]); s2[1] = fmaf(o.y, yp.y, s2[1]);
                s2[2] = fmaf(o.z, yp.z, s2[2]); s2[3] = fmaf(o.w, yp.w, s2[3]);
                buf_store4(rO, mine ? xvo + j * KC * 4u : kOOB, so, o, NT);  // rows past M: dropped by the bounds check
            }
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---- dW blocks over the tile's 32 rows (one k-step): A = X^T slots 16 w .., B = dY^T slots 16 nb .., two blocks at a time
        {
            const unsigned char *xsrc = Xb + (16 * wave) * 64 + trd + ((g4 ^ tswz(nn)) << 4);   // (16 w leaves the swizzle as it is)
            const bf16x8 ah = frag(*reinterpret_cast<const u32x4 *>(xsrc)), am = frag(*reinterpret_cast<const u32x4 *>(xsrc + PIECE)),
                         al = frag(*reinterpret_cast<const u32x4 *>(xsrc + 2 * PIECE));
            const unsigned char *tsrc = Tb + trd + ((g4 ^ tswz(nn)) << 4);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                bf16x8 bh[2], bm[2], bl[2];
                f32x4 smw[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const unsigned char *src = tsrc + (2 * q4 + b) * 16 * 64;
                    bh[b] = frag(*reinterpret_cast<const u32x4 *>(src));
                    bm[b] = frag(*reinterpret_cast<const u32x4 *>(src + PIECE));
                    bl[b] = frag(*reinterpret_cast<const u32x4 *>(src + 2 * PIECE));
                    smw[b] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#define PCOPS_BT_MM(A_, B_, C_, O_)                                                                 \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                   \
        C_[O_ + b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A_, B_[b], C_[O_ + b], 0, 0, 0)
                PCOPS_BT_MM(al, bh, smw, 0);
                PCOPS_BT_MM(ah, bl, smw, 0);
                PCOPS_BT_MM(am, bm, smw, 0);
                PCOPS_BT_MM(am, bh, smw, 0);
                PCOPS_BT_MM(ah, bm, smw, 0);
                PCOPS_BT_MM(ah, bh, accw, 2 * q4);
#undef PCOPS_BT_MM
#pragma unroll
                for (int b = 0; b < 2; ++b) accw[2 * q4 + b] += smw[b];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // One request in registers: a tile is staged, its raw Yprev kept, and the registers are asked again at once for the tile after
    // it -- in flight across the whole matrix phase.  Waves 0..3 stage, then compute; waves 4..7 compute, then stage.
    if (cnt > 0) {
        Req rq;
        float4 yk[2], yn[2];
        request(rq, grp);
        stage(rq, grp, lds);
        yk[0] = rq.x[0]; yk[1] = rq.x[1];
        request(rq, grp + ngrp);
        __syncthreads();
        // two half steps per tile, ONE copy of either phase (two copies of the request made the compiler shuffle the registers it
        // lands in across the loop edge, behind a vmcnt(0) on the loads just issued): half step s stages when s % 2 == hf
        for (int s = 0; s < 2 * cnt; ++s) {
            const int i = s >> 1, tile = grp + i * ngrp;
            if ((s & 1) == hf) {
                stage(rq, tile + ngrp, lds + ((i + 1) & 1) * IMG);
                // (the copy as opaque moves: a plain one is sunk behind the request and turned round -- the loads then land in other
                // registers and are copied into place at the loop edge, behind a wait on them)
                keep4(yn[0], rq.x[0]); keep4(yn[1], rq.x[1]);
                // (fenced: hoisted above the staging's last reads, the loads land in other registers and are copied at the loop
                // edge behind a wait on them)
                __builtin_amdgcn_sched_barrier(0);
                request(rq, tile + 2 * ngrp);
                __builtin_amdgcn_sched_barrier(0);
            } else {
                compute(tile, lds + (i & 1) * IMG, yk);
            }
            if (s & 1) {
                yk[0] = yn[0]; yk[1] = yn[1];
                __syncthreads();
            }
        }
    }

    // ---- the workgroup's partial: every sum in index order
    int te = tid;
    asm volatile("" : "+v"(te));
    const int enn = te & 15, eg4 = (te >> 4) & 3, ecq = 8 * ((te >> 5) & 3) + (te & 7), erg = 4 * (te >> 7) + ((te >> 3) & 3);
    const int eqd = te & 3;
    // dW: block nb, register r = slot row 16 w + 4 g4 + r, slot column 16 nb + nn; slot s is column 4 (s % 32) + s / 32
    float *out = part + (unsigned)grp * (KC * KC);
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
        const int sj = 16 * nb + enn, n = 4 * (sj & 31) + (sj >> 5);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int si = 16 * wave + 4 * eg4 + r, k = 4 * (si & 31) + (si >> 5);
            out[k * KC + n] = accw[nb][r];
        }
    }
    // statistics: the 16 row pairs of a quad in a fixed butterfly order
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int d = 4; d < 64; d <<= 1) {
            s1[e] += __shfl_xor(s1[e], d, 64);
            s2[e] += __shfl_xor(s2[e], d, 64);
        }
    }
    if ((te & 63) < 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gstats[((unsigned)grp * 2 + 0) * KC + 16 * wave + 4 * eqd + e] = s1[e];
            gstats[((unsigned)grp * 2 + 1) * KC + 16 * wave + 4 * eqd + e] = s2[e];
        }
    }
    if (dbpart) {
        float *sdb = reinterpret_cast<float *>(lds);                              // [16 row pairs][128 columns]
#pragma unroll
        for (int e = 0; e < 4; ++e) sdb[erg * KC + 4 * ecq + e] = dbs[e];
        __syncthreads();
        if (te < KC) {
            float v = 0.f;
            for (int r = 0; r < 16; ++r) v += sdb[r * KC + te];
            dbpart[(unsigned)grp * KC + te] = v;
        }
    }
}

// out[i] = the P partial copies of element i added in a fixed order (16 lanes of copies, then the lanes in index order): dW from
// the [P][K N] copies, db from the [P][N] copies behind them
__global__ __launch_bounds__(1024) void bwd_tiles128_sum_kernel(int P, const float *__restrict__ part, float *__restrict__ dW,
                                                                const float *__restrict__ dbpart, float *__restrict__ db) {
    __shared__ double sm[16][64];
    constexpr int NB1 = KC * KC / 64;
    const bool second = blockIdx.x >= NB1;
    const int len = second ? KC : KC * KC;
    const float *src = second ? dbpart : part;
    const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int i = (second ? (blockIdx.x - NB1) * 64 : blockIdx.x * 64) + c;
    double s = 0.0;
    for (int pp = pl; pp < P; pp += 16) s += (double)src[(long long)pp * len + i];
    sm[pl][c] = s;
    __syncthreads();
    if (pl == 0) {
        double tt = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) tt += sm[k][c];
        (second ? db : dW)[i] = (float)tt;
    }
}

}  // namespace

extern "C" {

// PCOPS_BWD_TILES128 = 1 (default): the query answers; 0: it answers 0 (kernel A/B only)
int pcops_mlp_bwd_tiles_groups(long long M, int K, int N) {
    static const bool on = pcops_env_switch("PCOPS_BWD_TILES128", true);
    if (!on || K != KC || N != KC || M < 2 * TR || M * (KC * 4) >= (1ll << 31)) return 0;
    const long long tiles = (M + TR - 1) / TR;
    return (int)(tiles < 256 ? tiles : 256);
}

int pcops_mlp_bwd_tiles_rows(long long M, int K, int N, const float *Yprev, const float *a_scale, const float *a_shift,
                             const float *G, const float *Y, const float *p, const float *q, const float *t, const float *W,
                             float *partial, float *dW, float *db, float *Gprev, float *stats_partial, const pcops_rows_t *rows,
                             pcops_stream_t stream) {
    PCOPS_REQUIRE_SHAPE(M >= 1 && K >= 1 && N >= 1);
    if (!Yprev || !a_scale || !a_shift || !G || !Y || !p || !q || !t || !W || !partial || !dW || !Gprev || !stats_partial)
        return PCOPS_ERR_NULL_POINTER;
    if (rows) {
        PCOPS_REQUIRE_PTR(rows->blocks); PCOPS_REQUIRE_PTR(rows->block_start); PCOPS_REQUIRE_PTR(rows->rows);
        if (reinterpret_cast<uintptr_t>(rows->blocks) & 15) return PCOPS_ERR_UNSUPPORTED;
    }
    const int groups = pcops_mlp_bwd_tiles_groups(M, K, N);
    if (groups == 0) return PCOPS_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(Yprev) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(Y) |
         reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(Gprev)) & 15)
        return PCOPS_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    float *dbpart = db ? partial + (long long)groups * KC * KC : nullptr;
    static const bool nt_on = pcops_env_switch("PCOPS_NT_STORE", true);   // as mlp.hip's outputs of 256 MB and more
    const bool nt = nt_on && M * (KC * 4) >= (256ll << 20);
    pcops_note_pipe(1);
    pcops_note_plan(18, 2, KC, 0, rows ? 4 : 0);
    auto launch = [&](auto kern) {
        return pcops_launch_lds(kern, dim3(groups), dim3(512), (size_t)LDS_BYTES, 160 * 1024, st, (int)M,
                                rows ? rows->rows : nullptr, rows ? static_cast<const RowBlock *>(rows->blocks) : nullptr, Yprev,
                                a_scale, a_shift, G, Y, p, q, t, W, partial, dbpart, Gprev, stats_partial);
    };
    const int rc = rows ? (nt ? launch(bwd_tiles128_kernel<true, true>) : launch(bwd_tiles128_kernel<true, false>))
                        : (nt ? launch(bwd_tiles128_kernel<false, true>) : launch(bwd_tiles128_kernel<false, false>));
    if (rc) return rc;
    hipLaunchKernelGGL(bwd_tiles128_sum_kernel, dim3(KC * KC / 64 + (db ? KC / 64 : 0)), dim3(1024), 0, st, groups, partial, dW,
                       dbpart, db);
    return pcops_launch_status();
}

}  // extern "C"
