// common.h -- shared host/device helpers of libpcops (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/pcops.h"
#include "device.h"

#define PCOPS_REQUIRE_PTR(p) \
    do { if ((p) == nullptr) return PCOPS_ERR_NULL_POINTER; } while (0)
#define PCOPS_REQUIRE_SHAPE(cond) \
    do { if (!(cond)) return PCOPS_ERR_BAD_SHAPE; } while (0)
#define PCOPS_REQUIRE_ARG(cond) \
    do { if (!(cond)) return PCOPS_ERR_BAD_ARGUMENT; } while (0)

// The two readers of the environment.  A switch that is on by default is turned off by a leading '0', one that is off by
// default is turned on by a leading '1'; anything else leaves the default.  Callers keep the value in a `static const`
// where it is to be read once per process.
static inline bool pcops_env_switch(const char *name, bool dflt) {
    const char *e = getenv(name);
    return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
}
static inline int pcops_env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

static inline int pcops_launch_status() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return PCOPS_OK;
    static const bool verbose = getenv("PCOPS_DEBUG_LAUNCH") != nullptr;      // what HIP said, on stderr
    if (verbose) fprintf(stderr, "libpcops: launch failed: %s (%s)\n", hipGetErrorString(e), hipGetErrorName(e));
    return PCOPS_ERR_LAUNCH;
}

static inline hipStream_t as_stream(pcops_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Zero `bytes` bytes at p on the stream: what the launchers that accumulate with atomics do to their output first.
// hipMemsetAsync, as ever -- unless the stream is being captured into a HIP graph (captured_step.py).  A captured
// hipMemsetAsync becomes a memset node, and on ROCm 7.0 such a node clears the whole range on the graph's first launch
// and only HALF of it on every later one (measured on the MI355X: 128 of 256 and 98 304 of 196 608 floats left as they
// were on the second and third replay; tests/test_captured_step_gpu.py replays one), so under capture the range is
// cleared by a kernel node instead.  Ranges that are not whole, aligned 32-bit words keep the memset.
static __global__ __launch_bounds__(256) void pcops_zero_kernel(unsigned *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
static inline hipError_t pcops_zero_async(void *p, size_t bytes, hipStream_t st) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (st == nullptr || bytes == 0 || (bytes & 3) || (reinterpret_cast<uintptr_t>(p) & 3) ||
        hipStreamIsCapturing(st, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusActive)
        return hipMemsetAsync(p, 0, bytes, st);
    const size_t n = bytes / 4;
    const unsigned grid = n < (size_t)4096 * 256 ? cdiv((long long)n, 256) : 4096u;
    hipLaunchKernelGGL(pcops_zero_kernel, dim3(grid), dim3(256), 0, st, static_cast<unsigned *>(p), n);
    return hipGetLastError();
}

// A kernel whose dynamic LDS may pass the 64 KB default: raise its ceiling to max_lds, launch it, and return the launch's
// status.  The attribute is set at every call; a refused attribute is PCOPS_ERR_LAUNCH.
template <typename... Params, typename... Args>
static inline int pcops_launch_lds(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, int max_lds, hipStream_t st,
                                   Args... args) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) !=
        hipSuccess)
        return PCOPS_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    return pcops_launch_status();
}

// A run-time value as a template argument: f(std::integral_constant<int, V>{}) for the V of Vs... that equals v, and its
// result; `otherwise` when none does.
template <int... Vs, typename F>
static inline int pcops_dispatch(int v, int otherwise, F &&f) {
    int rc = otherwise;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

extern "C" int pcops_get_deterministic(void);     // abi.hip: bit-reproducible backward passes requested
extern "C" int pcops_get_option(int option);      // abi.hip: the arithmetic options of pcops.h (read at every call)
void pcops_note_pipe(int pipe);                   // abi.hip: what pcops_last_launch_pipe() reports (0 fp32, 1 split bf16, 2 both)
void pcops_note_acc_stats(int on);                // abi.hip: what pcops_last_launch_acc_stats() reports (pcops_note_pipe clears it)
// abi.hip: what pcops_last_launch_plan() reports -- the variant the last product launch took (codes in pcops.h)
void pcops_note_plan(int path, int split, int bn, int wst, int pool);
void pcops_note_plan_field(int field, int value);   // one field of the plan just noted (a sub-launcher's own decision)

// xyz_bwd_tiles.hip: the form of pcops_mlp_bwd_fused_xyz_rows its kernel takes (uncompacted rows and a dense G are the caller's
// to check), and the launch -- buffers as bwd_fused_kernel's for `groups` workgroups, dW and db final
bool pcops_xyz_bwd_tiles_form(long long M, int K, int N);
int pcops_xyz_bwd_tiles_launch(long long M, int groups, const float *off4, const float *xyzw, const float *a_scale,
                               const float *a_shift, const float *G, const float *Y, const float *p, const float *q,
                               const float *t, const float *W, float *partial, float *dW, float *db, float *stats_partial,
                               float *xyz_stats, hipStream_t st);

// ---- what the translation units of the MLP family share (mlp.hip: the matrix products; mlp_bn.hip: the per-channel and
// elementwise passes around them; pooltop_sparse.hip: the sparse halves of the pooled top layer's algebraic backward)
namespace pcops_mlp {
constexpr int kBlk = 16;          // rows per block of a compacted row set
}  // namespace pcops_mlp
// a compacted row set as an argument of an entry point (NULL: all rows)
static inline int rows_ok(const pcops_rows_t *rows) {
    if (!rows) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(rows->blocks); PCOPS_REQUIRE_PTR(rows->block_start); PCOPS_REQUIRE_PTR(rows->rows);
    if (reinterpret_cast<uintptr_t>(rows->blocks) & 15) return PCOPS_ERR_UNSUPPORTED;
    return PCOPS_OK;
}
constexpr int kTopRowsWs = 512;   // workgroups (= partial copies) of pool_top_wsparse_rows_kernel
// what the two addend kernels over compacted rows need of the shape (the addend is indexed by the compacted row: at most M
// rows of Kp floats behind a 32-bit offset); pcops_mlp_pool_top_rows_supported (mlp.hip) adds what the other three calls need
static inline bool addend_rows_shape_ok(int M, int Kp, int N, int S) {
    return S % pcops_mlp::kBlk == 0 && S <= 128 && (Kp == 64 || Kp == 128) && N <= 256 && N % 32 == 0 &&
           (long long)M * Kp * 4 < (long long)kOOB;
}
// mlp_bn.hip: sum_partials2_kernel on the stream -- out [L] = the sum of the P copies part [P][L] and, when out2 is not NULL,
// out2 [L2] = that of part2 [P][L2], in a fixed order.  What closes every product kernel that writes a partial copy per workgroup.
#define PCOPS_HIDDEN __attribute__((visibility("hidden")))      // crosses translation units, not part of the C ABI
PCOPS_HIDDEN int pcops_mlp_sum_partials2(int P, long long L, const float *part, float *out, long long L2, const float *part2,
                                         float *out2, hipStream_t st);

constexpr int kWave = 64;  // CDNA wavefront

// Asymmetric STATIC wave priority (round 4; MI355X_MICROARCH.md "Two waves per SIMD").  Two co-resident waves that run
// the same [MFMA chain | VALU phase] loop at equal priority settle in LOCKSTEP: both contend for the matrix pipe (each
// chain takes twice as long), then both contend for the VALU issue slots -- time = MFMA + VALU, nothing overlaps,
// exactly the "matrix-pipe busy + 4.5 x other instructions" the round-2/3 counters showed.  With the odd wave slot of
// every SIMD at priority 1 its chain runs unimpeded while the partner waits, and from then on one wave's VALU phase
// sits under the other's MFMA chain.  PCOPS_WAVE_PRIO (compile time, A/B builds through PCOPS_LIB): bit 0 = the
// single-role kernels (gemm_ws, knn_mfma) by hardware wave slot, bit 1 = the consumer (MFMA) waves of the producer /
// consumer kernels.
#ifndef PCOPS_WAVE_PRIO
#define PCOPS_WAVE_PRIO 0
#endif
__device__ __forceinline__ void wave_prio_stagger() {
#if PCOPS_WAVE_PRIO & 1
    const unsigned slot = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);   // HW_REG_HW_ID.wave_id: slot on the SIMD
    if (slot & 1) __builtin_amdgcn_s_setprio(1);
#endif
}
__device__ __forceinline__ void wave_prio_consumer(bool consumer) {
#if PCOPS_WAVE_PRIO & 2
    if (consumer) __builtin_amdgcn_s_setprio(1);
#else
    (void)consumer;
#endif
}

// unsigned max across the 64 lanes of a wave, wave-uniform result.  DPP row shifts + the two gfx9 row broadcasts
// (a max-"scan" whose last lane holds the total): 6 VALU instructions and one v_readlane, no LDS round trips.
// (The bpermute butterfly this replaces cost 12 ds_bpermute with ~100 cycles of latency each per 64-bit key --
// most of an FPS round.)  Lanes a step does not reach see 0, the identity of an unsigned max.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    auto step = [&](auto ctrl, auto rmask) {
        const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, decltype(ctrl)::value, decltype(rmask)::value,
                                                                 0xf, true);
        v = o > v ? o : v;
    };
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});   // row_shr:1
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});   // row_shr:2
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});   // row_shr:4
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});   // row_shr:8
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});   // row_bcast:15 -> rows 1, 3
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});   // row_bcast:31 -> rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// 64-bit max across the 64 lanes of a wave (all lanes get the result): the high words first, then the low words
// of the lanes that hold the winning high word.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)(v & 0xffffffffu);
    const unsigned mh = wave_max_u32(hi);
    const unsigned ml = wave_max_u32(hi == mh ? lo : 0u);
    return ((unsigned long long)mh << 32) | ml;
}

// ---- XCD-aware numbering of workgroups (round 5).  Workgroup `bid` (linear dispatch order) of `nwg` runs on XCD bid % 8
// (observed, MI355X_MICROARCH.md "Workgroup dispatch" -- a speed assumption only, nothing may depend on it): renumber so
// that every XCD owns a CONTIGUOUS range of the virtual ids (bijective for any nwg).  Kernels that deal several
// workgroups to one cloud use it to keep a cloud's rows in ONE L2 instead of fetching them into all eight.
__device__ __forceinline__ unsigned xcd_contiguous(unsigned bid, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7u, x = bid & 7u, i = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}
// a (parts-per-cloud, clouds) grid: the (part, cloud) this workgroup takes, all parts of a cloud on one XCD
struct CloudPart { int part, cloud; };
__device__ __forceinline__ CloudPart xcd_cloud_part() {
    const unsigned vb = xcd_contiguous(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const unsigned cloud = vb / gridDim.x;
    return CloudPart{(int)(vb - cloud * gridDim.x), (int)cloud};
}
