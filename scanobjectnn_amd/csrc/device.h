// device.h -- the device vocabulary of libpcops: one name per vector shape, the split of an fp32 operand into three bf16
// pieces, buffer-resource addressing.  Included by common.h.  The first block compiles as plain C++17 without a HIP header
// (tests/test_split_operands_cpu.py builds the split on the host and pins it bit for bit).
#pragma once

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline
#endif

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// fp32 -> three bf16 pieces, x = h + m + l up to 2^-25 |x| (each residual is exact in fp32; round-to-nearest pieces carry
// their own signs, so 3 x 8 significant bits cover the 24 of the operand; below 2^-100 the residuals turn denormal and the
// identity holds to an absolute 2^-133 instead).  Products of two pieces are exact in fp32.  (tests/test_split_operands_cpu.py)
// Written on PAIRS of values (round 6): one v_cvt_pk_bf16_f32 per pair and piece, the widening as shift / mask of the packed word,
// the residuals as v_pk_add_f32 -- 36 instructions for eight values.  As a loop over single values hipcc paired what it could and
// left 46 (17 conversions, ten of the sixteen subtractions unpacked); same arithmetic, bit for bit.
__host__ __device__ __forceinline__ void split3_pair(float a, float b, bf16x2 &h, bf16x2 &m, bf16x2 &l) {
    const f32x2 v = {a, b};
    h = __builtin_convertvector(v, bf16x2);
    const f32x2 r1 = v - __builtin_convertvector(h, f32x2);
    m = __builtin_convertvector(r1, bf16x2);
    const f32x2 r2 = r1 - __builtin_convertvector(m, f32x2);
    l = __builtin_convertvector(r2, bf16x2);
}
// the same as three packed words (value a in the low half)
__host__ __device__ __forceinline__ void split3_pair(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
    bf16x2 hh, mm, ll;
    split3_pair(a, b, hh, mm, ll);
    h = __builtin_bit_cast(unsigned, hh); m = __builtin_bit_cast(unsigned, mm); l = __builtin_bit_cast(unsigned, ll);
}

#ifdef __HIPCC__
__device__ __forceinline__ void split3(const float4 &x0, const float4 &x1, bf16x8 &h, bf16x8 &m, bf16x8 &l) {
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        bf16x2 hh, mm, ll;
        split3_pair(x[2 * p], x[2 * p + 1], hh, mm, ll);
        h[2 * p] = hh.x; h[2 * p + 1] = hh.y;
        m[2 * p] = mm.x; m[2 * p + 1] = mm.y;
        l[2 * p] = ll.x; l[2 * p + 1] = ll.y;
    }
}
// eight values as the three pieces of one MFMA fragment
__device__ __forceinline__ void split3_frag(const float (&x)[8], u32x4 &h, u32x4 &m, u32x4 &l) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned a, b, c;
        split3_pair(x[2 * k], x[2 * k + 1], a, b, c);
        h[k] = a; m[k] = b; l[k] = c;
    }
}
__device__ __forceinline__ bf16x8 frag(const u32x4 &v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ f32x16 zero16() {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// ---- buffer-resource addressing (gfx950): ONE 32-bit VGPR offset per lane + a scalar offset per access, and the
// hardware bounds check (offset >= num_records -> loads return 0, stores are dropped) replaces every row guard.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, long long bytes) {
    const unsigned n = bytes <= 0 ? 0u : (bytes > 0xFFFFFFFFll ? 0xFFFFFFFFu : (unsigned)bytes);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, n, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_u32(const void *base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    // (aux 2 = non-temporal on the streamed operand reads: SSG 23.05 vs 23.05 k, DGCNN 9.85 vs 9.85 k -- nothing; stores: see buf_store4)
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ unsigned buf_load1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
// nt: non-temporal (aux bit 1 on gfx94x / gfx950): the output is a stream far larger than the L2 and the memory-side cache
// that nothing reads back soon -- not allocating its lines measured 7 % on a pure 2.7 GB write stream (edgeconv.hip MODE 1)
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, float4 x, bool nt = false) {
    u32x4 v;
    v.x = __float_as_uint(x.x); v.y = __float_as_uint(x.y); v.z = __float_as_uint(x.z); v.w = __float_as_uint(x.w);
    if (nt) __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, 2);
    else __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, 0);
    // gfx950 store-data hazard hipcc does not pad: a VALU write to the data registers of a 16-byte buffer store in the
    // very next issue slot still reaches the store (observed: the .w word of the last four lanes of every 16-lane group
    // took the NEXT row's value whenever a v_pk_add_f32 rewrote v[n+2:n+3] right behind the store).  LLVM's recogniser
    // only pads MUBUF stores WITHOUT an SGPR soffset; these use one.  The statement below reads the four registers, so
    // nothing can be allocated into them before it, and it carries the wait states itself.  (Round 2 met the same
    // corruption when it unrolled the MFMA loop and put it down to a code-generation accident.)
    asm volatile("s_nop 1" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w) : "memory");
}
constexpr unsigned kOOB = 0x7FFFFFF0u;   // a voffset no tensor reaches: forces the bounds check to fail
#endif
