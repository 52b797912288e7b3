// feed.hip -- the device-resident feed (pcops.h "Device-resident feed"): one launch builds a step's
// batch from the set on the device.  The cloud, the points taken from it and every random number are functions of
// (seed, epoch, step, position in the epoch's order, output point): counter-based Philox4x32-10, no generator state, so the
// launch is the same graph node on every replay while `params` (device memory) moves from step to step.
//
// Shape: a workgroup of 256 lanes builds 256 consecutive output points of one row.  The reads are scattered 12-byte
// gathers (one point per lane); the writes are contiguous: the 256 x 3 floats go through LDS (lane stride 3, coprime to the
// bank count) and leave as whole 1-KiB wave stores.  What is uniform over a cloud -- the eight round keys of its permutation,
// its rotation's cos / sin or its scales and translations -- is computed by four lanes (one Philox block each) ahead of the
// points, not per point.
#include "common.h"

namespace {

constexpr int kFeedBlock = 256;
constexpr float kTwoPi = 6.28318530717958647692f;

struct U4 { unsigned w0, w1, w2, w3; };

__device__ __forceinline__ U4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

// ((w >> 9) + 0.5) 2^-23: 2 k + 1 < 2^24, so every step is exact
__device__ __forceinline__ float uniform01(unsigned w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__device__ __forceinline__ unsigned feistel_f(unsigned v, unsigned k, unsigned w) {
    v ^= k;
    v *= 0x9E3779B1u;
    v ^= v >> 15;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    return v & ((1u << w) - 1u);
}

// the cloud's permutation at j < ni.  Cycle walking ends: the network permutes [0, 2^bits), and the cycle through j
// comes back to j itself, which is below ni.
__device__ __forceinline__ unsigned feed_perm(unsigned j, unsigned ni, const unsigned *key) {
    const unsigned nbits = ni > 1u ? 32u - (unsigned)__clz((int)(ni - 1u)) : 0u;      // bit_length(ni - 1), ni < 2^31
    const unsigned bits = nbits < 2u ? 2u : nbits;
    const unsigned a = bits >> 1, b = bits - a;
    unsigned x = j;
    do {
        unsigned L = x >> b, R = x & ((1u << b) - 1u), wl = a, wr = b;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned t = L ^ feistel_f(R, key[r], wl);
            L = R;
            R = t;
            const unsigned w = wl;
            wl = wr;
            wr = w;
        }
        x = (L << b) | R;
    } while (x >= ni);
    return x;
}

__global__ __launch_bounds__(kFeedBlock) void feed_batch_kernel(
    int K, long long ntot, int n, int mode, int recipe, const float *__restrict__ pts, const long long *__restrict__ offsets,
    const long long *__restrict__ labels, const long long *__restrict__ side, const int *__restrict__ order,
    const int *__restrict__ idx_pts, const int *__restrict__ params, unsigned k0, unsigned k1, float sigma, float clip,
    float smin, float smax, float tval, float *__restrict__ x, long long *__restrict__ y, long long *__restrict__ m) {
    __shared__ unsigned s_key[8];
    __shared__ float s_cloud[8];
    __shared__ float s_x[kFeedBlock * 3];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int j0 = blockIdx.x * kFeedBlock, j = j0 + tid;
    const int cnt = n - j0 < kFeedBlock ? n - j0 : kFeedBlock;
    const int first = params[0], step = params[1], epoch = params[2];
    const long long g = (long long)first + r;
    const size_t out0 = (size_t)r * (size_t)n + (size_t)j0;          // first output point of this workgroup
    const bool lead = blockIdx.x == 0 && tid == 0;

    int c = -1;
    if (g >= 0 && g < (long long)K) c = order[g];
    long long base = 0, ni = 0;
    if (c >= 0 && c < K) {
        base = offsets ? offsets[c] : (long long)c * ntot;
        ni = offsets ? offsets[c + 1] - base : ntot;
    }
    if (ni < (long long)n || ni > 0x7fffffffLL) {                    // past the end (or outside the contract): zeros, label -1
        for (int i = tid; i < cnt * 3; i += kFeedBlock) x[out0 * 3 + i] = 0.0f;
        if (m != nullptr && side != nullptr && tid < cnt) m[out0 + tid] = 0;
        if (lead) y[r] = -1;
        return;
    }

    if (tid < 2) {
        if (mode == 1) {
            const U4 k = philox4x32_10((unsigned)c, (unsigned)epoch, (unsigned)tid, PCOPS_FEED_TAG_PERM, k0, k1);
            s_key[4 * tid + 0] = k.w0;
            s_key[4 * tid + 1] = k.w1;
            s_key[4 * tid + 2] = k.w2;
            s_key[4 * tid + 3] = k.w3;
        }
    } else if (tid < 4 && recipe != 0) {
        const U4 d = philox4x32_10((unsigned)g, (unsigned)step, (unsigned)(tid - 2), PCOPS_FEED_TAG_CLOUD, k0, k1);
        if (recipe == 1) {
            if (tid == 2) {
                const float theta = kTwoPi * uniform01(d.w0);
                s_cloud[0] = cosf(theta);
                s_cloud[1] = sinf(theta);
            }
        } else if (tid == 2) {
            const float span = smax - smin;
            s_cloud[0] = smin + span * uniform01(d.w0);
            s_cloud[1] = smin + span * uniform01(d.w1);
            s_cloud[2] = smin + span * uniform01(d.w2);
        } else {
            s_cloud[4] = (2.0f * uniform01(d.w0) - 1.0f) * tval;
            s_cloud[5] = (2.0f * uniform01(d.w1) - 1.0f) * tval;
            s_cloud[6] = (2.0f * uniform01(d.w2) - 1.0f) * tval;
        }
    }
    __syncthreads();

    if (tid < cnt) {
        const unsigned src = mode == 1 ? feed_perm((unsigned)j, (unsigned)ni, s_key) : (unsigned)idx_pts[j];
        float vx = 0.0f, vy = 0.0f, vz = 0.0f;
        long long sv = 0;
        if (src < (unsigned)ni) {
            const size_t p = (size_t)base + src;
            vx = pts[p * 3 + 0];
            vy = pts[p * 3 + 1];
            vz = pts[p * 3 + 2];
            if (side != nullptr) sv = side[p];
        }
        if (recipe == 1) {
            const float cs = s_cloud[0], sn = s_cloud[1];
            const float rx = vx * cs - vz * sn, rz = vx * sn + vz * cs;
            vx = rx;
            vz = rz;
        } else if (recipe == 2) {
            vx = vx * s_cloud[0] + s_cloud[4];
            vy = vy * s_cloud[1] + s_cloud[5];
            vz = vz * s_cloud[2] + s_cloud[6];
        }
        if (recipe != 0) {
            const U4 w = philox4x32_10((unsigned)g, (unsigned)step, (unsigned)j, PCOPS_FEED_TAG_JIT, k0, k1);
            const float r0 = sqrtf(-2.0f * logf(uniform01(w.w0))), a0 = kTwoPi * uniform01(w.w1);
            const float r2 = sqrtf(-2.0f * logf(uniform01(w.w2))), a2 = kTwoPi * uniform01(w.w3);
            vx = vx + fminf(fmaxf(sigma * (r0 * cosf(a0)), -clip), clip);
            vy = vy + fminf(fmaxf(sigma * (r0 * sinf(a0)), -clip), clip);
            vz = vz + fminf(fmaxf(sigma * (r2 * cosf(a2)), -clip), clip);
        }
        s_x[tid * 3 + 0] = vx;
        s_x[tid * 3 + 1] = vy;
        s_x[tid * 3 + 2] = vz;
        if (m != nullptr && side != nullptr) m[out0 + tid] = sv;
    }
    if (lead) y[r] = labels[c];
    __syncthreads();
    for (int i = tid; i < cnt * 3; i += kFeedBlock) x[out0 * 3 + i] = s_x[i];
}

// the step's parameters into device memory: plain stores of launch arguments (the pattern of TFAdam.set_lr's fill)
__global__ void feed_set_params_kernel(int first, int step, int epoch, int *__restrict__ params) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        params[0] = first;
        params[1] = step;
        params[2] = epoch;
        params[3] = 0;
    }
}

}  // namespace

extern "C" int pcops_feed_set_params(int first, int step, int epoch, int *params, pcops_stream_t stream) {
    PCOPS_REQUIRE_PTR(params);
    hipLaunchKernelGGL(feed_set_params_kernel, dim3(1), dim3(64), 0, as_stream(stream), first, step, epoch, params);
    return pcops_launch_status();
}

extern "C" int pcops_feed_batch(int K, long long ntot, int B, int n, int mode, int recipe, long long min_points,
                                const float *pts, const long long *offsets, const long long *labels, const long long *side,
                                const int *order, const int *idx_pts, const int *params, unsigned long long seed, float sigma,
                                float clip, float smin, float smax, float tval, float *x, long long *y, long long *m,
                                pcops_stream_t stream) {
    const bool dense = offsets == nullptr;
    PCOPS_REQUIRE_SHAPE(K > 0 && n > 0 && B >= 0 && (!dense || ntot > 0));
    PCOPS_REQUIRE_SHAPE((long long)n <= min_points && (!dense || min_points <= ntot));
    PCOPS_REQUIRE_ARG((mode == 0 || mode == 1) && recipe >= 0 && recipe <= 2 && (mode == 1 || dense));
    PCOPS_REQUIRE_ARG(recipe == 0 || clip > 0.0f);
    PCOPS_REQUIRE_ARG(recipe != 2 || smin <= smax);
    if (B > 65535) return PCOPS_ERR_UNSUPPORTED;
    if (B == 0) return PCOPS_OK;
    PCOPS_REQUIRE_PTR(pts); PCOPS_REQUIRE_PTR(labels); PCOPS_REQUIRE_PTR(order); PCOPS_REQUIRE_PTR(params);
    PCOPS_REQUIRE_PTR(x); PCOPS_REQUIRE_PTR(y);
    if (mode == 0) PCOPS_REQUIRE_PTR(idx_pts);
    hipLaunchKernelGGL(feed_batch_kernel, dim3(cdiv(n, kFeedBlock), B), dim3(kFeedBlock), 0, as_stream(stream), K, ntot, n,
                       mode, recipe, pts, offsets, labels, side, order, idx_pts, params, (unsigned)(seed & 0xffffffffull),
                       (unsigned)(seed >> 32), sigma, clip, smin, smax, tval, x, y, m);
    return pcops_launch_status();
}
