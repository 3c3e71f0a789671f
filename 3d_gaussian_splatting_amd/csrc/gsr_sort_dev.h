// gsr_sort_dev.h -- device helpers that more than one of gsr_radix.hip, gsr_binning.hip and
// gsr_tilesort.hip uses.  Device code only; in an unnamed namespace, so each kernel file keeps its
// own internal copies, as when they were one file.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {
namespace {

// One wave writes LDS words that other lanes of the same wave then read (or the reverse): no
// block barrier is needed, only that the compiler and the LDS queue keep the order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lanes of the wave below this one
__device__ inline uint64_t lanemask_lt() {
    const int lane = threadIdx.x & 63;
    return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

// live item count: the host bound, or the device count clamped to it
__device__ __forceinline__ long long live_count(long long cap, const uint32_t* __restrict__ n_dev) {
    if (!n_dev) return cap;
    const long long n = (long long)*n_dev;
    return n < cap ? n : cap;
}

// lanes (among `active`) holding the same digit as this lane (digits of up to MAXB bits)
template <int MAXB = 8>
__device__ inline uint64_t match_digit(uint32_t d, int nbits, uint64_t active) {
    uint64_t peers = active;
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        if (b < nbits) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
    }
    return peers;
}

}  // namespace
}  // namespace gsr
