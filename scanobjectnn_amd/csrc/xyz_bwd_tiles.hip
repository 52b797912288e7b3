// xyz_bwd_tiles.hip -- the one-pass backward of a 64 -> 64 layer that sits on the ARITHMETIC first layer (SA1's second layer),
// uncompacted rows, dense G:  pcops_mlp_bwd_fused_xyz_rows at K == N == 64 (mlp.hip dispatches).
//
//   y1 = fmaf(dz, w2, fmaf(dy, w1, fmaf(dx, w0, b)))   the first layer, rebuilt from 16 bytes of offsets per row
//   z  = fmaf(y1, a_scale, a_shift),  X1 = max(z, 0),  m1 = z > 0
//   dY = fmaf(p, G, fmaf(q, Y, t))
//   dW = X1^T dY,  db = 1^T dY,  Gp = m1 . (dY W^T);   out: dW, db and the column sums of Gp, Gp y1, off_i Gp (nothing per row)
//
// bwd_fused_kernel (mlp.hip) runs this shape with four producer and four consumer waves; the pass follows the four consumers.
// Here all eight waves of a workgroup do the same work, in two halves of four waves:
//   * a step is 128 rows, half hf takes its 64-row tile 2 step + hf; steps are dealt to the workgroups in ascending order
//   * STAGE: thread (column quad cq, row group rg) of a half holds four rows x four columns of G and Y in registers (requested a
//     step ahead, unconditional buffer loads, 32-bit offsets; rows past M read as zeros), forms dY once, adds it to its db sums, splits it
//     into three bf16 pieces once and stores the pieces twice: row-major R (the A operand of dX) and transposed T (the B operand
//     of dW).  Both are [piece][64][8 units of 16 bytes], the unit XORed with the low bits of the row / slot, so that the
//     staging stores and the 16-byte fragment reads are both conflict free without padding.  Column c of dY is T's slot
//     16 (c % 4) + c / 4 (a thread's four columns fall into four different bank groups).
//   * COMPUTE: wave (rb, kb) of a half owns rows 32 rb .. of the tile and channels 32 kb .. of the layer below:
//       dX block [32 rows][32 channels] = dY W^T: 4 k-steps x 6 v_mfma_f32_32x32x16_bf16; W^T's pieces are ready fragments in LDS,
//         split once per workgroup (in registers they were 48 VGPRs a wave and 208 bytes of scratch)
//       dW block [32 channels][64 columns] over ITS 32 rows: 2 k-steps x 2 column blocks x 6; the A operand is built in registers
//         in fragment layout from the tile's offsets in LDS (broadcast reads) and the channel's six coefficients
//       The k index of the dW product is a row, and any order of the rows serves: k-step t, lane half h, element j is row
//       32 rb + 16 t + 8 (j / 4) + 4 h + j % 4 -- exactly the rows of the lane's dX accumulator elements 8 t + j.  So y1, z and
//       the offsets a lane has just used for the A operand are the ones its epilogue needs: the mask, the five column sums
//       follow the k-step in registers, no second rebuild and no second read.
//     The dW block of a wave covers its own 32 rows only (the two row blocks and the two halves are added once, at the end, in
//     a fixed order): every wave builds the A operand for 32 rows instead of 64.
//   * the halves run one phase apart (half 1 starts with a barrier of its own): while one half stages -- vector and LDS-store
//     work -- the other is in its matrix phase, and a SIMD holds one wave of each.
// Large (h h) and small products in separate accumulators (the split and the buffer loads are device.h's);
// the small ones join the large once per tile.
// No float atomics; every sum has a fixed order: two calls give the same bits.
#include "common.h"

namespace {

constexpr int KC = 64;                         // K == N == 64
constexpr int TR = 64;                         // rows of a tile
constexpr int PIECE = TR * 128;                // bytes of one piece of R or T
constexpr int HALF = 6 * PIECE + 3 * TR * 4;   // R, T, the tile's offsets as [x | y | z][64]: 49 920 bytes per half
constexpr int WF_OFF = 2 * HALF;               // W^T's pieces as ready B fragments [piece][k-step][channel block][lane] x 16 bytes
constexpr int CO_OFF = WF_OFF + 3 * 8 * 64 * 16;   // p, q, t [64] each
constexpr int LDS_BYTES = CO_OFF + 3 * KC * 4;
constexpr int STAT_OFF = 8 * 2048 * 4;         // the final sums: dW copies [8 waves][2][32][32], then the statistics, then db
constexpr int DB_OFF = STAT_OFF + 8 * 5 * 32 * 4;

struct Req {
    float4 g[4], y[4], o;          // the thread's four rows of G and Y (one column quad), one row of offsets
};

__global__ __launch_bounds__(512, 1) void xyz_bwd_tiles_kernel(int M, const float *__restrict__ off4, const float *__restrict__ xw,
                                                               const float *__restrict__ asc, const float *__restrict__ ash,
                                                               const float *__restrict__ G, const float *__restrict__ Y,
                                                               const float *__restrict__ p, const float *__restrict__ q,
                                                               const float *__restrict__ t, const float *__restrict__ W,
                                                               float *__restrict__ part, float *__restrict__ dbpart,
                                                               float *__restrict__ gstats, float *__restrict__ xstats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hf = wave >> 2, rb = (wave >> 1) & 1, kb = wave & 1;
    const int ht = tid & 255, cq = ht & 15, rg = ht >> 4;
    const int ntiles = (M + TR - 1) / TR, nsteps = (ntiles + 1) / 2;
    const int grp = blockIdx.x, ngrp = gridDim.x;
    const int cnt = grp < nsteps ? (nsteps - grp + ngrp - 1) / ngrp : 0;          // steps of this workgroup

    unsigned char *Rb = lds + hf * HALF, *Tb = Rb + 3 * PIECE;
    float *offl = reinterpret_cast<float *>(Tb + 3 * PIECE);                      // [3][64]
    u32x4 *wf = reinterpret_cast<u32x4 *>(lds + WF_OFF);
    float *cdy = reinterpret_cast<float *>(lds + CO_OFF);

    // ---- once per workgroup: W^T's pieces as the B operand of dX -- element j of lane (l32, h) at k-step ks, channel block cb is
    // W[32 cb + l32][16 ks + 8 h + j] (one fragment per thread) -- and p, q, t
    {
        const float *src = W + (32 * ((tid >> 6) & 1) + l32) * KC + 16 * (tid >> 7) + 8 * h;
        const float4 f0 = *reinterpret_cast<const float4 *>(src), f1 = *reinterpret_cast<const float4 *>(src + 4);
        const float wv[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
        u32x4 fh, fm, fl;
        split3_frag(wv, fh, fm, fl);
        wf[tid] = fh; wf[512 + tid] = fm; wf[1024 + tid] = fl;
        if (tid < KC) { cdy[tid] = p[tid]; cdy[KC + tid] = q[tid]; cdy[2 * KC + tid] = t[tid]; }
    }
    __syncthreads();
    const int ch = 32 * kb + l32;                                                 // the lane's channel of the layer below
    const float w0 = xw[ch], w1 = xw[KC + ch], w2 = xw[2 * KC + ch], bb = xw[3 * KC + ch], sc = asc[ch], sh = ash[ch];
    const u32x4 *wfa = wf + kb * 64 + lane;                                       // + 128 ks, + 512 piece
    f32x16 accw[2] = {zero16(), zero16()};                                        // dW block, carried over every tile
    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    float s1 = 0.f, s2 = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;                       // sums of Gp, Gp y1, off_i Gp of channel ch

    // ---- addresses that do not change
    // T: slot s = 16 e + cq of column 4 cq + e; rows 4 rg .. 4 rg + 3 are elements 4 ((rg / 2) % 2) .. of unit 2 (rg / 4) + rg % 2
    const int tU = 2 * (rg >> 2) + (rg & 1);
    const int twr = cq * 128 + ((tU ^ (cq & 7)) << 4) + 8 * ((rg >> 1) & 1);      // + 16 e * 128 (16 e % 8 == 0: the same swizzle)
    // R: row 4 rg + j, columns 4 cq .. 4 cq + 3 are half cq % 2 of unit cq / 2, stored at unit (cq / 2) ^ (row % 8) = ru ^ j
    const int rbase = 4 * rg * 128 + 8 * (cq & 1), ru = ((cq >> 1) ^ (4 * (rg & 1))) << 4;
    const int arow = 32 * rb + l32;                                               // dX: the lane's row of the A operand
    const int ard = arow * 128, arx = arow & 7;                                   // unit 2 ks + h at ((2 ks + h) ^ arx) << 4
    const int trd = l32 * 128, trx = l32 & 7;                                     // dW: slot 32 nb + l32, unit 2 (2 rb + t) + h

    // One descriptor per tensor and one 32-bit offset per thread: the tile's first row is a scalar offset, a thread's rows
    // immediates.  A row past M is out of the descriptor's range and reads as zeros (M 256 bytes < 2^31: the launcher).
    const __amdgpu_buffer_rsrc_t rG = make_rsrc_u32(G, (unsigned)M * (KC * 4u)), rY = make_rsrc_u32(Y, (unsigned)M * (KC * 4u)),
                                 rO = make_rsrc_u32(off4, (unsigned)M * 16u);
    const unsigned gvo = (unsigned)(4 * rg * KC + 4 * cq) * 4u, ovo = (unsigned)(ht & 63) * 16u;
    auto request = [&](Req &r, int step) {
        const int tile = 2 * step + hf;
        const unsigned row0 = (unsigned)(tile < ntiles ? tile : ntiles - 1) * TR;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r.g[j] = buf_load4(rG, gvo + j * KC * 4u, row0 * (KC * 4u));
            r.y[j] = buf_load4(rY, gvo + j * KC * 4u, row0 * (KC * 4u));
        }
        r.o = buf_load4(rO, ovo, row0 * 16u);
    };

    // FULL: all 64 rows of the tile exist -- thread-uniform, true for every tile but the last; a row past M is a zero row of dY,
    // which is an exact zero in every sum (its X1 and y1 are finite: its offsets read as zeros)
    auto stage_ = [&](const Req &r, int row0, auto full_) {
        constexpr bool FULL = decltype(full_)::value;
        const float4 cp = *reinterpret_cast<const float4 *>(cdy + 4 * cq), cqv = *reinterpret_cast<const float4 *>(cdy + KC + 4 * cq),
                     ct = *reinterpret_cast<const float4 *>(cdy + 2 * KC + 4 * cq);
        float d[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 g = r.g[j], y = r.y[j];
            d[j][0] = fmaf(cp.x, g.x, fmaf(cqv.x, y.x, ct.x));
            d[j][1] = fmaf(cp.y, g.y, fmaf(cqv.y, y.y, ct.y));
            d[j][2] = fmaf(cp.z, g.z, fmaf(cqv.z, y.z, ct.z));
            d[j][3] = fmaf(cp.w, g.w, fmaf(cqv.w, y.w, ct.w));
            if (!FULL && !(row0 + 4 * rg + j < M)) d[j][0] = d[j][1] = d[j][2] = d[j][3] = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) dbs[e] += d[j][e];
        }
        unsigned ph[4][2], pm[4][2], pl[4][2];                                    // [column][row pair]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            split3_pair(d[0][e], d[1][e], ph[e][0], pm[e][0], pl[e][0]);
            split3_pair(d[2][e], d[3][e], ph[e][1], pm[e][1], pl[e][1]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                             // T: four rows of one column per store
            unsigned char *dst = Tb + twr + e * 16 * 128;
            *reinterpret_cast<u32x2 *>(dst) = u32x2{ph[e][0], ph[e][1]};
            *reinterpret_cast<u32x2 *>(dst + PIECE) = u32x2{pm[e][0], pm[e][1]};
            *reinterpret_cast<u32x2 *>(dst + 2 * PIECE) = u32x2{pl[e][0], pl[e][1]};
        }
        auto lo = [](unsigned a, unsigned b) { return (a & 0xffffu) | (b << 16); };     // the pairs' first rows, two columns
        auto hi = [](unsigned a, unsigned b) { return (a >> 16) | (b & 0xffff0000u); };  // their second rows
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {                                          // R: four columns of one row per store
            unsigned char *d0 = Rb + rbase + 2 * pr * 128 + (ru ^ (2 * pr << 4)), *d1 = Rb + rbase + (2 * pr + 1) * 128 + (ru ^ ((2 * pr + 1) << 4));
            *reinterpret_cast<u32x2 *>(d0) = u32x2{lo(ph[0][pr], ph[1][pr]), lo(ph[2][pr], ph[3][pr])};
            *reinterpret_cast<u32x2 *>(d0 + PIECE) = u32x2{lo(pm[0][pr], pm[1][pr]), lo(pm[2][pr], pm[3][pr])};
            *reinterpret_cast<u32x2 *>(d0 + 2 * PIECE) = u32x2{lo(pl[0][pr], pl[1][pr]), lo(pl[2][pr], pl[3][pr])};
            *reinterpret_cast<u32x2 *>(d1) = u32x2{hi(ph[0][pr], ph[1][pr]), hi(ph[2][pr], ph[3][pr])};
            *reinterpret_cast<u32x2 *>(d1 + PIECE) = u32x2{hi(pm[0][pr], pm[1][pr]), hi(pm[2][pr], pm[3][pr])};
            *reinterpret_cast<u32x2 *>(d1 + 2 * PIECE) = u32x2{hi(pl[0][pr], pl[1][pr]), hi(pl[2][pr], pl[3][pr])};
        }
        if (ht < TR) { offl[ht] = r.o.x; offl[TR + ht] = r.o.y; offl[2 * TR + ht] = r.o.z; }
    };

    auto compute = [&]() {
        // ---- dX block = dY W^T
        // (every k-step's fragments are requested one k-step ahead and the scheduler is fenced per k-step: left to itself it
        // requests all of them up front and spills the next tile's request)
        f32x16 accd = zero16(), smd = zero16();
        const unsigned char *rsrc = Rb + ard;
        u32x4 na[3], nw[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
            na[pc] = *reinterpret_cast<const u32x4 *>(rsrc + ((h ^ arx) << 4) + pc * PIECE);
            nw[pc] = wfa[512 * pc];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 ah = frag(na[0]), am = frag(na[1]), al = frag(na[2]);
            const bf16x8 bh = frag(nw[0]), bm = frag(nw[1]), bl = frag(nw[2]);
            if (ks + 1 < 4) {
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    na[pc] = *reinterpret_cast<const u32x4 *>(rsrc + (((2 * (ks + 1) + h) ^ arx) << 4) + pc * PIECE);
                    nw[pc] = wfa[512 * pc + 128 * (ks + 1)];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            smd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, smd, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, accd, 0, 0, 0);
            smd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, smd, 0, 0, 0);
            smd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, smd, 0, 0, 0);
            smd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, smd, 0, 0, 0);
            smd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, smd, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        accd += smd;                                     // (here: sixteen registers less under the dW k-steps)
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW block over the wave's 32 rows, and the epilogue of the rows a k-step has just rebuilt.  The small products of a
        // tile are summed apart and join the block once per tile (carried across tiles they were 32 registers under the staging)
        f32x16 smw[2] = {zero16(), zero16()};
#pragma unroll
        for (int ts = 0; ts < 2; ++ts) {
            // rows r0 .. r0 + 3 and r0 + 8 .. r0 + 11: one 16-byte read per coordinate and row quad, the same address in a lane half
            const float *orow = offl + 32 * rb + 16 * ts + 4 * h;
            const float4 ox0 = *reinterpret_cast<const float4 *>(orow), ox1 = *reinterpret_cast<const float4 *>(orow + 8);
            const float4 oy0 = *reinterpret_cast<const float4 *>(orow + TR), oy1 = *reinterpret_cast<const float4 *>(orow + TR + 8);
            const float4 oz0 = *reinterpret_cast<const float4 *>(orow + 2 * TR), oz1 = *reinterpret_cast<const float4 *>(orow + 2 * TR + 8);
            const float ox[8] = {ox0.x, ox0.y, ox0.z, ox0.w, ox1.x, ox1.y, ox1.z, ox1.w};
            const float oy[8] = {oy0.x, oy0.y, oy0.z, oy0.w, oy1.x, oy1.y, oy1.z, oy1.w};
            const float oz[8] = {oz0.x, oz0.y, oz0.z, oz0.w, oz1.x, oz1.y, oz1.z, oz1.w};
            float y1[8], z[8], x1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                y1[j] = fmaf(oz[j], w2, fmaf(oy[j], w1, fmaf(ox[j], w0, bb)));
                z[j] = fmaf(y1[j], sc, sh);
                x1[j] = fmaxf(z[j], 0.f);
            }
            u32x4 xh, xm, xl;
            split3_frag(x1, xh, xm, xl);
            const bf16x8 ah = frag(xh), am = frag(xm), al = frag(xl);
            const unsigned char *src = Tb + trd + (((2 * (2 * rb + ts) + h) ^ trx) << 4);
            bf16x8 bh[2], bm[2], bl[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                bh[nb] = frag(*reinterpret_cast<const u32x4 *>(src + nb * 32 * 128));
                bm[nb] = frag(*reinterpret_cast<const u32x4 *>(src + nb * 32 * 128 + PIECE));
                bl[nb] = frag(*reinterpret_cast<const u32x4 *>(src + nb * 32 * 128 + 2 * PIECE));
            }
            // one product at a time over the two column blocks: consecutive matrix instructions do not share an accumulator
#define PCOPS_XT_MM(A_, B_, C_)                                                                     \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                                \
        C_[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_, B_[nb], C_[nb], 0, 0, 0)
            PCOPS_XT_MM(al, bh, smw);
            PCOPS_XT_MM(ah, bl, smw);
            PCOPS_XT_MM(am, bm, smw);
            PCOPS_XT_MM(am, bh, smw);
            PCOPS_XT_MM(ah, bm, smw);
            PCOPS_XT_MM(ah, bh, accw);
#undef PCOPS_XT_MM
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float gv = z[j] > 0.f ? accd[8 * ts + j] : 0.f;
                s1 += gv;
                s2 = fmaf(gv, y1[j], s2);
                sx = fmaf(ox[j], gv, sx);
                sy = fmaf(oy[j], gv, sy);
                sz = fmaf(oz[j], gv, sz);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        accw[0] += smw[0]; accw[1] += smw[1];
    };

    auto do_step = [&](int step, Req &cur, Req &nxt) {
        request(nxt, step + ngrp);
        const int row0 = (2 * step + hf) * TR;
        if (row0 + TR <= M) stage_(cur, row0, std::true_type{});
        else stage_(cur, row0, std::false_type{});
        __syncthreads();
        // the matrix phase at priority 1: its wave shares a SIMD with a staging wave of the other half, whose vector work then
        // fills the gaps instead of delaying the fragment reads in front of a matrix chain (measured)
        __builtin_amdgcn_s_setprio(1);
        compute();
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();
    };
    Req ra, rq;
    request(ra, grp);
    if (hf) __syncthreads();                                                      // half 1 runs one phase behind half 0
    for (int i = 0; i < cnt; i += 2) {
        do_step(grp + i * ngrp, ra, rq);
        if (i + 1 < cnt) do_step(grp + (i + 1) * ngrp, rq, ra);
    }
    if (!hf) __syncthreads();

    // ---- the workgroup's partial: every sum in index order
    // (indices taken from an opaque copy of the thread number: computed before the loop they were carried through it in scratch)
    int te = tid;
    asm volatile("" : "+v"(te));
    const int el32 = te & 31, eh = (te >> 5) & 1, ecq = te & 15, erg = (te >> 4) & 15;
    __syncthreads();
    float *red = reinterpret_cast<float *>(lds);                                  // [wave][column block][32 channels][32 slots]
    float *sst = reinterpret_cast<float *>(lds + STAT_OFF);                       // [wave][5][32 channels]
    float *sdb = reinterpret_cast<float *>(lds + DB_OFF);                         // [half][row group][64 columns]
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            red[wave * 2048 + nb * 1024 + (8 * (i >> 2) + 4 * eh + (i & 3)) * 32 + el32] = accw[nb][i];
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    sx += __shfl_xor(sx, 32, 64); sy += __shfl_xor(sy, 32, 64); sz += __shfl_xor(sz, 32, 64);
    if (eh == 0) {
        float *d = sst + wave * 5 * 32 + el32;
        d[0] = s1; d[32] = s2; d[64] = sx; d[96] = sy; d[128] = sz;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sdb[(hf * 16 + erg) * KC + 4 * ecq + e] = dbs[e];
    __syncthreads();
    // wave hf 4 + rb 2 + kb holds channels 32 kb ..; its copies are added in the order (half 0, rows 0), (0, 1), (1, 0), (1, 1)
    float *out = part + (unsigned)grp * (KC * KC);
    for (int i = te; i < KC * KC; i += 512) {
        const int k = i >> 6, n = i & 63, s = 16 * (n & 3) + (n >> 2);            // column n lives in slot s
        const float *src = red + (k >> 5) * 2048 + (s >> 5) * 1024 + (k & 31) * 32 + (s & 31);
        out[i] = ((src[0] + src[2 * 2048]) + src[4 * 2048]) + src[6 * 2048];
    }
    if (te < 5 * KC) {
        const int which = te >> 6, c = te & 63;
        const float *src = sst + (c >> 5) * 5 * 32 + which * 32 + (c & 31);
        const float v = ((src[0] + src[2 * 5 * 32]) + src[4 * 5 * 32]) + src[6 * 5 * 32];
        if (which < 2) gstats[((unsigned)grp * 2 + which) * KC + c] = v;
        else xstats[((unsigned)grp * 3 + which - 2) * KC + c] = v;
    }
    if (dbpart && te < KC) {
        float v = 0.f;
        for (int r = 0; r < 32; ++r) v += sdb[r * KC + te];
        dbpart[(unsigned)grp * KC + te] = v;
    }
}

// out[i] = the P partial copies of element i added in a fixed order (16 lanes of copies, then the lanes in index order): dW from
// the [P][K N] copies, db from the [P][N] copies behind them
__global__ __launch_bounds__(1024) void xyz_bwd_tiles_sum_kernel(int P, const float *__restrict__ part, float *__restrict__ dW,
                                                                 const float *__restrict__ dbpart, float *__restrict__ db) {
    __shared__ double sm[16][64];
    constexpr int NB1 = KC * KC / 64;
    const bool second = blockIdx.x >= NB1;
    const int len = second ? KC : KC * KC;
    const float *src = second ? dbpart : part;
    const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int i = (second ? 0 : blockIdx.x * 64) + c;
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

// PCOPS_BWD_XYZ_TILES = 1 (default): the form above takes this kernel; 0: bwd_fused_kernel for every shape
bool pcops_xyz_bwd_tiles_form(long long M, int K, int N) {
    static const bool on = pcops_env_switch("PCOPS_BWD_XYZ_TILES", true);   // kernel A/B only
    return on && K == KC && N == KC && M >= 65536 && M * KC * 4 < (long long)kOOB;
}

int pcops_xyz_bwd_tiles_launch(long long M, int groups, const float *off4, const float *xyzw, const float *a_scale,
                               const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                               const float *t, const float *W, float *partial, float *dW, float *db, float *stats_partial,
                               float *xyz_stats, hipStream_t st) {
    float *dbpart = db ? partial + (long long)groups * KC * KC : nullptr;
    pcops_note_pipe(1);
    pcops_note_plan(17, 2, KC, 0, 0);
    const int rc = pcops_launch_lds(xyz_bwd_tiles_kernel, dim3(groups), dim3(512), (size_t)LDS_BYTES, 160 * 1024, st, (int)M, off4,
                                    xyzw, a_scale, a_shift, G, Y, p, q, t, W, partial, dbpart, stats_partial, xyz_stats);
    if (rc) return rc;
    hipLaunchKernelGGL(xyz_bwd_tiles_sum_kernel, dim3(KC * KC / 64 + (db ? 1 : 0)), dim3(1024), 0, st, groups, partial, dW, dbpart,
                       db);
    return pcops_launch_status();
}
