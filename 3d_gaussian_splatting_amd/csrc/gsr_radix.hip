// gsr_radix.hip -- the global LSD radix sort of (u32 key, u32 value) pairs on gfx950: the tile-key
// sort of the emitted instances (radix binning) and the presort's 32-bit depth-key sort.
//
// Reduce-then-scan per digit of up to 8 bits: upsweep (per-block digit counts), column scan (per
// digit over blocks), downsweep (stable wave64 ranking: 8 ballots give each lane its peer mask,
// popcount below it is its rank in the round; per-wave running counters in LDS; digit base =
// scanned counts).  All integer work: HBM / issue-bound, no MFMA.  The live count can stay on the
// device (n_dev): every kernel is launched for the capacity and clamps to it.
#include "gsr_kernels.h"
#include "gsr_sort_dev.h"

namespace gsr {
namespace {

constexpr int kB = kSortBlock;  // 256 threads = 4 waves
constexpr int kWaves = kB / 64;

// Chunk of the key array a radix block works on.  Blocks are dealt to the 8 XCDs round-robin
// (b % 8), so neighbouring chunks would sit in different L2s; with the remap each XCD takes a
// contiguous run of chunks, and the partial 64-B lines at the ends of a chunk's digit runs (the
// downsweep's scatter) and of its histogram column entries meet their neighbours' halves in the
// same L2 before write-back.
// (1M / 1080p tile sort 0.1145 -> 0.102 ms, 5M 0.496 -> 0.475; the same remap of the per-tile
// depth sort's tiles measured no change.)
__device__ __forceinline__ int radix_chunk(int b, int nb) {
    const int q = nb / 8, r = nb % 8, xcd = b % 8, local = b / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

// ---- upsweep: per-block digit histogram, written digit-major hist[d * nb + b] ----
// Counting needs no stable rank, so per-wave LDS sub-histograms with atomics suffice (the
// 8-ballot peer match of the downsweep measured slower here).  Blocks past the live count
// write zero columns.
// RI: rounds of 64 keys per wave (kRadixItems, or kRadixItemsSmall for small sorts)
template <int RI>
__global__ __launch_bounds__(kB) void radix_upsweep(const uint32_t* __restrict__ keys, long long cap,
                                                    const uint32_t* __restrict__ n_dev, int shift, int nbits,
                                                    int nb, uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[kWaves][256];
    const int tid = threadIdx.x, w = tid >> 6;
    const long long n = live_count(cap, n_dev);
#pragma unroll
    for (int k = 0; k < kWaves; ++k) cnt[k][tid] = 0;
    __syncthreads();
    const uint32_t mask = (1u << nbits) - 1u;
    const int chunk = radix_chunk(blockIdx.x, nb);
    const long long base = (long long)chunk * (kB * RI) + (long long)w * (64 * RI);
    // all RI loads in flight before the first atomic (one HBM round trip per wave, not RI / 4)
    uint32_t k[RI];
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const long long idx = base + r * 64 + (tid & 63);
        k[r] = idx < n ? keys[idx] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const long long idx = base + r * 64 + (tid & 63);
        if (idx < n) atomicAdd(&cnt[w][(k[r] >> shift) & mask], 1u);
    }
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += cnt[k][tid];
    hist[(size_t)tid * nb + chunk] = s;
}

// ---- column scan: block d turns hist[d*nb .. +nb) into an exclusive scan; totals[d] ----
// Four consecutive counts per thread per round (1024 per block round: 8 rounds for the 7936
// blocks of a 5M / 1080p tile sort instead of 31).
constexpr int kColQ = 4;
__global__ __launch_bounds__(kB) void radix_colscan(uint32_t* __restrict__ hist, int nb,
                                                    uint32_t* __restrict__ totals) {
    __shared__ uint32_t wsum[kWaves];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    uint32_t* col = hist + (size_t)blockIdx.x * nb;
    uint32_t carry = 0;
    for (int base = 0; base < nb; base += kB * kColQ) {
        const int i0 = base + tid * kColQ;
        uint32_t v[kColQ], sv = 0;
#pragma unroll
        for (int q = 0; q < kColQ; ++q) {
            v[q] = i0 + q < nb ? col[i0 + q] : 0u;
            sv += v[q];
        }
        // inclusive wave scan of the per-thread sums
        uint32_t x = sv;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t pre = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) pre += (k < w) ? wsum[k] : 0u;
        uint32_t run = carry + pre + x - sv;
#pragma unroll
        for (int q = 0; q < kColQ; ++q) {
            if (i0 + q < nb) col[i0 + q] = run;
            run += v[q];
        }
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) tot += wsum[k];
        __syncthreads();
        carry += tot;
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

// ---- downsweep: stable scatter, reordered through LDS so global writes are coalesced ----
template <int RI>
__global__ __launch_bounds__(kB) void radix_downsweep(const uint32_t* __restrict__ keys_in,
                                                      const uint32_t* __restrict__ vals_in,
                                                      uint32_t* __restrict__ keys_out,
                                                      uint32_t* __restrict__ vals_out, long long cap,
                                                      const uint32_t* __restrict__ n_dev, int shift, int nbits,
                                                      int nb, const uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ totals) {
    __shared__ uint32_t wcnt[kWaves][256];
    __shared__ uint32_t gbase[256];   // global position of this block's first item of digit d
    __shared__ uint32_t lbase[256];   // block-local position of the first item of digit d
    __shared__ uint32_t wsum[kWaves];
    constexpr int TILE = kB * RI;
    __shared__ uint32_t skey[TILE];
    __shared__ uint32_t sval[TILE];
    const long long n = live_count(cap, n_dev);
    const int chunk = radix_chunk(blockIdx.x, nb);
    const long long bbase = (long long)chunk * TILE;
    if (bbase >= n) return;  // block-uniform: nothing of this block is live
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t mask = (1u << nbits) - 1u;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) wcnt[k][tid] = 0;
    // global digit base: exclusive scan of totals + this block's scanned count
    {
        const uint32_t v = totals[tid];
        uint32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t pre = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) pre += (k < w) ? wsum[k] : 0u;
        gbase[tid] = pre + x - v + hist[(size_t)tid * nb + chunk];
    }
    __syncthreads();
    const long long base = bbase + (long long)w * (64 * RI);
    uint32_t key[RI], val[RI], rank[RI];
    const uint64_t lt = lanemask_lt();
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const long long idx = base + r * 64 + lane;
        const bool valid = idx < n;
        key[r] = valid ? keys_in[idx] : 0xFFFFFFFFu;
        val[r] = valid ? (vals_in ? vals_in[idx] : (uint32_t)idx) : 0u;
    }
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const long long idx = base + r * 64 + lane;
        const bool valid = idx < n;
        const uint32_t d = (key[r] >> shift) & mask;
        const uint64_t active = __ballot(valid);
        const uint64_t peers = match_digit(d, nbits, active);
        const uint32_t old = wcnt[w][d];
        rank[r] = old + (uint32_t)__popcll(peers & lt);
        if (valid && (peers & lt) == 0) wcnt[w][d] = old + (uint32_t)__popcll(peers);
    }
    __syncthreads();
    {
        // per digit: wave prefixes (in place) and the block count; block-local digit starts
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const uint32_t t = wcnt[k][tid];
            wcnt[k][tid] = c;
            c += t;
        }
        uint32_t x = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        __syncthreads();  // wsum reuse
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t pre = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) pre += (k < w) ? wsum[k] : 0u;
        lbase[tid] = pre + x - c;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const long long idx = base + r * 64 + lane;
        if (idx < n) {
            const uint32_t d = (key[r] >> shift) & mask;
            const uint32_t lp = lbase[d] + wcnt[w][d] + rank[r];
            skey[lp] = key[r];
            sval[lp] = val[r];
        }
    }
    __syncthreads();
    const int count = (n - bbase) < TILE ? (int)(n - bbase) : TILE;
#pragma unroll 4
    for (int i = tid; i < count; i += kB) {
        const uint32_t k = skey[i];
        const uint32_t d = (k >> shift) & mask;
        const uint32_t pos = gbase[d] + (uint32_t)i - lbase[d];
        keys_out[pos] = k;
        vals_out[pos] = sval[i];
    }
}

}  // namespace

int radix_sort(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* k0, uint32_t* v0,
               uint32_t* k1, uint32_t* v1, long long cap, const uint32_t* n_dev, int nbits, uint32_t* hist,
               int* which, hipStream_t s) {
    *which = -1;
    if (cap <= 0) return 0;
    const int nb = radix_blocks(cap);
    uint32_t* totals = hist + (size_t)256 * (nb + 1);
    const uint32_t* kin = keys_in;
    const uint32_t* vin = vals_in;
    int dst = 0;
    // the fewest 8-bit-or-narrower passes, digits split evenly (13 tile bits: 7 + 6, not 8 + 5:
    // half the buckets in the first pass, so each block's runs to scatter are twice as long;
    // 0.114 vs 0.120 ms at 1M / 1080p, 0.486 vs 0.512 at 5M)
    const int passes = (nbits + 7) / 8, per = (nbits + passes - 1) / passes;
    for (int shift = 0; shift < nbits; shift += per) {
        const int bits = (nbits - shift) < per ? (nbits - shift) : per;
        uint32_t* ko = dst == 0 ? k0 : k1;
        uint32_t* vo = dst == 0 ? v0 : v1;
        if (radix_tile_for(cap) == kRadixTile) {
            hipLaunchKernelGGL(radix_upsweep<kRadixItems>, dim3(nb), dim3(kB), 0, s, kin, cap, n_dev, shift, bits, nb,
                               hist);
            hipLaunchKernelGGL(radix_colscan, dim3(256), dim3(kB), 0, s, hist, nb, totals);
            hipLaunchKernelGGL(radix_downsweep<kRadixItems>, dim3(nb), dim3(kB), 0, s, kin, vin, ko, vo, cap, n_dev,
                               shift, bits, nb, hist, totals);
        } else {
            hipLaunchKernelGGL(radix_upsweep<kRadixItemsSmall>, dim3(nb), dim3(kB), 0, s, kin, cap, n_dev, shift, bits,
                               nb, hist);
            hipLaunchKernelGGL(radix_colscan, dim3(256), dim3(kB), 0, s, hist, nb, totals);
            hipLaunchKernelGGL(radix_downsweep<kRadixItemsSmall>, dim3(nb), dim3(kB), 0, s, kin, vin, ko, vo, cap,
                               n_dev, shift, bits, nb, hist, totals);
        }
        kin = ko;
        vin = vo;
        *which = dst;
        dst ^= 1;
    }
    return (int)hipGetLastError();
}

}  // namespace gsr
