// gsr_train_dev.h -- the pieces the training-step translation units share (gsr_loss.hip,
// gsr_optim.hip, gsr_pointset.hip): the step guard, the float4 accessors, the geometry and the
// loop of a stream over an image plane, the fixed-order reductions, and the host's alignment test
// and kernel<true> / kernel<false> dispatch.  Each is stated here once.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "gsr_internal.h"

namespace gsr {

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// float4 accesses need every pointer at 16 bytes (a null pointer is aligned)
inline bool all_aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

// The device-side step guard: a render under a binning bound whose true instance count K (the
// scan's device counter) exceeded the bound was truncated; the optimizer step / statistics of
// that iteration are then dropped here, on the device, with no host wait (the host learns of
// the overflow one iteration later from its pinned copy and re-sizes).
__device__ __forceinline__ bool guard_tripped(const uint32_t* k, uint32_t cap) {
    return k != nullptr && *k > cap;  // written by an earlier kernel of the stream
}

// Streaming (non-temporal) loads / stores: parameters, gradients and moments are touched once per
// step, so they should not displace the L2 / MALL lines the rasterizer reuses.  Measured in the
// configs[4] loop (6M Gaussians, 1280x832, 4000 iterations): 89.8 vs 87.2 iters/s; two float4
// columns per thread: 87.6 (profiles/r04_experiments/loop_ab_4k.txt).
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float* p, float4 v) {
    const f32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
}

// V4: a full group of 4 elements on a 16-byte-aligned array (one float4 access); otherwise
// `cnt` <= 4 elements with scalar accesses, zeros loaded past them.
template <bool V4>
__device__ __forceinline__ void load4(const float* p, long long e0, int cnt, float (&v)[4]) {
    if (V4) {
        const float4 q = *reinterpret_cast<const float4*>(p + e0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[e0 + k] : 0.f;
    }
}

template <bool V4>
__device__ __forceinline__ void store4(float* p, long long e0, int cnt, const float (&v)[4]) {
    if (V4) {
        *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) p[e0 + k] = v[k];
    }
}

// A stream over a plane of n pixels: a block takes chunks of 256 x 4 consecutive pixels, chunk c
// of block b being b + c * gridDim.x, and the grid depends on n alone, so the partial sums and
// their order -- hence the bits -- are a function of the inputs only.
constexpr int kPlaneBlock = 256, kPlaneChunk = 4 * kPlaneBlock, kPlaneMaxBlocks = 2048;
__host__ __device__ inline long long plane_chunks(long long n) { return (n + kPlaneChunk - 1) / kPlaneChunk; }
inline int plane_blocks(long long n) {
    const long long c = plane_chunks(n);
    return (int)(c < kPlaneMaxBlocks ? (c > 0 ? c : 1) : kPlaneMaxBlocks);
}

// body(V4, e0, cnt) for each group of this thread, V4 a std::bool_constant.  VEC: every plane is
// 16-byte aligned, so the full groups of 4 move as float4 (V4 true); otherwise, and for the
// plane's last, partial group, the same thread moves the same pixels with scalar accesses, so
// both paths sum alike.
template <bool VEC, class Body>
__device__ __forceinline__ void for_each_plane_group(long long n, Body body) {
    const long long chunks = plane_chunks(n);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long e0 = c * kPlaneChunk + 4 * (long long)threadIdx.x;
        const long long left = n - e0;
        if (left <= 0) continue;
        if (VEC && left >= 4)
            body(std::true_type{}, e0, 4);
        else
            body(std::false_type{}, e0, left < 4 ? (int)left : 4);
    }
}

// launches a plane-stream kernel's float4 or scalar instantiation: launch_plane(vec, k<true>, k<false>, ...)
template <class K, class... Args>
inline void launch_plane(bool vec, K vec_kernel, K scalar_kernel, long long n, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(vec ? vec_kernel : scalar_kernel, dim3(plane_blocks(n)), dim3(kPlaneBlock), 0, s, args...);
}

// fixed-order block reduction of two values (256 threads, red[8]); thread 0 holds the sums
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * wv] = a;
        red[2 * wv + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (red[0] + red[2]) + (red[4] + red[6]);
        b = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

// The one-block (256 threads) reduction of nparts partials of N columns, the determinism contract
// of every loss sum: partial i is part[N i .. N i + N - 1]; each thread sums its partials (i = thread,
// thread + 256, ...) in double in index order, then a fixed 128..1 tree across threads.  On return
// r[k][0] is column k's sum, visible to every thread.
template <int N>
__device__ __forceinline__ void finalize_partials(const float* part, int nparts, double (&r)[N][256]) {
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += (double)part[N * (long long)i + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) r[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < N; ++k) r[k][threadIdx.x] += r[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

}  // namespace gsr
