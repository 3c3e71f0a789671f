// gsr_tilesort.hip -- per-tile depth order on gfx950: every tile's slice of the tile-grouped
// instance list sorted by (depth key, gid): the canonical (tile, depth bits, gid) order without a
// global depth sort.  Three forms, picked by launch_tile_depth_sort from the mean slice length,
// each handing what it cannot take to the next through a device queue:
//   - one wave per tile, the slice in VGPRs (tile_depth_wave: <= 1024 entries on 32-bit truncated
//     keys; tile_depth_wave_queue: <= 2048 on 64-bit keys): a bitonic network over DPP / swizzle /
//     bpermute exchanges, no barrier;
//   - one block of 4 or 8 waves per tile (tile_depth_block<NW>, tile_depth_block_queue: <= 4096 /
//     8192 entries): each wave the same network on 1024 entries, the runs merged through LDS;
//   - tile_depth_sort_big for the rest: a 1024-thread stable LDS radix sort of up to 16384 entries
//     (radix_sort_slice), longer slices in chunks merged by a bitonic network (global + LDS).
// The register forms sort distinct (depth, gid) keys, whatever order a slice arrives in; the radix
// form is stable and needs gid order in the slice, or its tie fix-up (`unordered`).
#include "gsr_kernels.h"
#include "gsr_sort_dev.h"

namespace gsr {
namespace {

// ---- the LDS radix sort of one slice (tile_depth_sort_big's whole-slice and chunk sort) ----
// A slice in gid order needs only a stable LSD sort of the 32-bit depth keys to end in (depth,
// gid) order.  Each pass is ranked as radix_downsweep ranks (wave64 ballot peer match, per-wave
// digit counters, a digit-major block scan), in LDS; passes whose digit is equal for every key are
// skipped.  Latency-bound per block (dependent LDS counter updates, ~6 syncs per pass).
// Wave w owns the contiguous run [w * 64 I, (w + 1) * 64 I) of the slice [rg.x, rg.y) of
// n <= NT * I entries, ranked round by round in index order (stable).  Ends with every LDS access
// behind a barrier, so a block may call it again for another slice.

// Runs of equal depth keys in a depth-sorted slice (skey, sval in LDS, n entries) into gid order.
// The thread holding a run's first entry sorts the run by insertion when it is at most
// kTieRunMax long (runs are disjoint, so no two threads touch the same entries); if any run is
// longer, the whole slice goes through an all-ascending bitonic network on the 64-bit (depth,
// gid) keys in place (a degenerate slice: many Gaussians at one depth).  Ends behind a barrier.
constexpr int kTieRunMax = 32;
__device__ __forceinline__ void tie_fixup(uint32_t* skey, uint32_t* sval, int n, int nt) {
    int longrun = 0;
    for (int i = threadIdx.x; i + 1 < n; i += nt) {
        const uint32_t k = skey[i];
        if (skey[i + 1] != k || (i > 0 && skey[i - 1] == k)) continue;  // not a run start
        int e = i + 2;
        while (e < n && skey[e] == k && e - i <= kTieRunMax) ++e;
        if (e - i > kTieRunMax) {
            longrun = 1;
            continue;
        }
        for (int a = i + 1; a < e; ++a) {  // insertion sort of (skey, sval)[i, e) by the 64-bit pair
            const uint32_t ka = skey[a], va = sval[a];
            const uint64_t x = ((uint64_t)ka << 32) | va;
            int b = a;
            while (b > i && ((((uint64_t)skey[b - 1]) << 32) | sval[b - 1]) > x) {
                skey[b] = skey[b - 1];
                sval[b] = sval[b - 1];
                --b;
            }
            skey[b] = ka;
            sval[b] = va;
        }
    }
    if (!__syncthreads_or(longrun)) return;
    int m = 1;
    while (m < n) m <<= 1;
    auto cex = [&](int i, int j) {  // i < j; j >= n is +inf padding
        if (j >= n) return;
        const uint64_t a = ((uint64_t)skey[i] << 32) | sval[i], b = ((uint64_t)skey[j] << 32) | sval[j];
        if (a > b) {
            skey[i] = (uint32_t)(b >> 32), sval[i] = (uint32_t)b;
            skey[j] = (uint32_t)(a >> 32), sval[j] = (uint32_t)a;
        }
    };
    for (int size = 2; size <= m; size <<= 1) {
        for (int d = size >> 1; d >= 1; d >>= 1) {
            const bool flip = d == (size >> 1);
            for (int t = threadIdx.x; t < (m >> 1); t += nt) {
                const int i = ((t & ~(d - 1)) << 1) | (t & (d - 1));
                cex(i, flip ? (i ^ (size - 1)) : (i + d));
            }
            __syncthreads();
        }
    }
}

// the one shape in use: 1024 threads, 16 items each (16384 keys), 8-bit digits
constexpr int kSliceNT = 1024, kSliceI = 16, kSliceDB = 8;
struct SliceLds {
    uint32_t wcnt[kSliceNT / 64][1 << kSliceDB];
    uint32_t lbase[1 << kSliceDB];
    uint32_t red[2][kSliceNT / 64];
    uint32_t skey[kSliceNT * kSliceI];
    uint32_t sval[kSliceNT * kSliceI];
};

__device__ __forceinline__ void radix_sort_slice(const uint2 rg, const uint32_t* __restrict__ depth_key,
                                                 uint32_t* __restrict__ gid, SliceLds& lds, bool unordered = false) {
    constexpr int NT = kSliceNT, I = kSliceI, DB = kSliceDB;
    constexpr int NWV = NT / 64, BINS = 1 << DB;
    constexpr uint32_t DMASK = BINS - 1u;
    auto& wcnt = lds.wcnt;
    auto& lbase = lds.lbase;
    auto& red = lds.red;
    auto& skey = lds.skey;
    auto& sval = lds.sval;
    const int n = (int)(rg.y - rg.x);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    // wave w owns [w * per, (w + 1) * per): per = the slice split evenly over the waves in whole
    // 64-lane rounds (<= 64 I since n <= CAP)
    const int per = (n + NWV * 64 - 1) / (NWV * 64) * 64;
    const int base = w * per;
    const int end = base + per < n ? base + per : n;
    uint32_t key[I], val[I], rank[I];
    uint32_t kor = 0u, kand = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < I; ++r) {
        const int idx = base + r * 64 + lane;
        const bool valid = idx < end;
        val[r] = valid ? gid[rg.x + idx] : 0u;
        key[r] = valid ? depth_key[val[r]] : 0xFFFFFFFFu;
        if (valid) {
            kor |= key[r];
            kand &= key[r];
        }
    }
    // bits where the slice's keys differ: passes over constant digits are no-ops (stable)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kor |= __shfl_xor(kor, o, 64);
        kand &= __shfl_xor(kand, o, 64);
    }
    if (lane == 0) {
        red[0][w] = kor;
        red[1][w] = kand;
    }
    __syncthreads();
    uint32_t diff = 0u;
    {
        uint32_t o_ = 0u, a_ = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < NWV; ++k) {
            o_ |= red[0][k];
            a_ &= red[1][k];
        }
        diff = o_ ^ a_;
    }
    const uint64_t lt = lanemask_lt();
    // The (stable) depth passes alone: a gid-ordered slice ends in (depth, gid) order.  An
    // unordered one (the row-bucketed binning leaves a tile's entries in arbitrary order) ends in
    // depth order with each run of equal depth keys in arbitrary gid order; tie_fixup puts
    // those runs in gid order afterwards (ties are rare and short: an LSD pass over the gid bits
    // per 8-9 of them would cost as much as the depth passes again).
    const int hb = diff ? 31 - __clz(diff) : 0;  // the highest differing bit
    bool ran = false;
    for (int shift = 0; shift < 32 && shift <= hb; shift += DB) {
        if (((diff >> shift) & DMASK) == 0u) continue;  // block-uniform
        ran = true;
        for (int d = tid; d < NWV * BINS; d += NT) (&wcnt[0][0])[d] = 0u;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < I; ++r) {
            if (base + r * 64 >= end) break;  // wave-uniform: only the rounds holding keys
            const int idx = base + r * 64 + lane;
            const bool valid = idx < end;
            const uint32_t d = (key[r] >> shift) & DMASK;
            const uint64_t peers = match_digit<DB>(d, DB, __ballot(valid));
            const uint32_t old = wcnt[w][d];
            rank[r] = old + (uint32_t)__popcll(peers & lt);
            if (valid && (peers & lt) == 0) wcnt[w][d] = old + (uint32_t)__popcll(peers);
        }
        __syncthreads();
        // per digit: wave prefixes in place, then the digit-major block scan -> lbase
        for (int d = tid; d < BINS; d += NT) {
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < NWV; ++k) {
                const uint32_t t = wcnt[k][d];
                wcnt[k][d] = c;
                c += t;
            }
            lbase[d] = c;
        }
        __syncthreads();
        if (tid < 64) {  // exclusive scan of the BINS digit totals, BINS / 64 per lane
            constexpr int Q = BINS / 64;
            uint32_t c4[Q], s4 = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                c4[q] = lbase[Q * tid + q];
                s4 += c4[q];
            }
            uint32_t x = s4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            uint32_t run = x - s4;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                lbase[Q * tid + q] = run;
                run += c4[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < I; ++r) {
            const int idx = base + r * 64 + lane;
            if (idx < end) {
                const uint32_t d = (key[r] >> shift) & DMASK;
                const uint32_t lp = lbase[d] + wcnt[w][d] + rank[r];
                skey[lp] = key[r];
                sval[lp] = val[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < I; ++r) {
            const int idx = base + r * 64 + lane;
            if (idx < end) {
                key[r] = skey[idx];
                val[r] = sval[idx];
            }
        }
        __syncthreads();  // skey / sval / wcnt are rewritten by the next pass
    }
    if (unordered && n > 1) {
        if (!ran) {  // every key equal: the slice is one run, in LDS for the fix-up
#pragma unroll
            for (int r = 0; r < I; ++r) {
                const int idx = base + r * 64 + lane;
                if (idx < end) {
                    skey[idx] = key[r];
                    sval[idx] = val[r];
                }
            }
            __syncthreads();
        }
        tie_fixup(skey, sval, n, NT);
        for (int i = tid; i < n; i += NT) gid[rg.x + i] = sval[i];
        __syncthreads();  // skey / sval / red[] are rewritten by the next slice
        return;
    }
#pragma unroll
    for (int r = 0; r < I; ++r) {
        const int idx = base + r * 64 + lane;
        if (idx < end) gid[rg.x + idx] = val[r];
    }
    __syncthreads();  // red[] is rewritten by the next slice
}

// ---- per-tile depth order, register form: one wave per tile ----
// A slice of n <= 64 E entries (E = 1 .. 16, the smallest power of two that holds it)
// is sorted by one wave in VGPRs as 64-bit (depth << 32 | gid) keys with a bitonic network: lane l
// holds entries l E .. l E + E - 1, so exchanges at distances below E stay inside a lane and the
// rest go lane to lane by DPP (lane xor 1 / 2 / 3, row mirrors, row_ror 8), ds_swizzle (xor 4,
// 16, 31 inside 32-lane halves) and ds_bpermute (across the halves).  The gid in the low word
// makes every key distinct, so the result is the canonical (depth, gid) order whatever order the
// slice arrives in (no stability needed), and there is no LDS, no barrier and no per-pass
// histogram: ~log2(64 E)^2 / 2 compare-exchange stages of 5-6 VALU ops per key pair.
// "Flip" network (every merge ascending: its first stage pairs i with i ^ (k - 1), mirrored).

// x from lane (lane ^ M) of the wave, M = 2^a - 1 (mirror stages) or 2^a (half cleaners)
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x) {
    static_assert(M >= 1 && M <= 63, "lane_xor distance");
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);
    else if constexpr (M == 3) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x1B, 0xF, 0xF, false);
    else if constexpr (M == 7) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, false);
    else if constexpr (M == 15) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, false);
    else if constexpr (M == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, false);
    else if constexpr (M == 4 || M == 16 || M == 31)  // bit mode: and 0x1f, xor M, inside 32-lane halves
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1F | (M << 10));
    else return (uint32_t)__shfl_xor((int)x, M, 64);  // 32, 63: across the halves
}

template <int M>
__device__ __forceinline__ uint64_t lane_xor(uint64_t x) {
    return ((uint64_t)lane_xor<M>((uint32_t)(x >> 32)) << 32) | lane_xor<M>((uint32_t)x);
}

// flip = 0: keep min(a, b); flip = ~0: keep max(a, b).  Keys are below 2^63 (a positive float's
// bits over a gid; padding 2^63 - 1), so the sign of a - b orders them; the select is a bit
// insert on that sign -- VALU only (a compare into an SGPR mask and a scalar XOR with the lane
// side would put a VALU -> SALU -> VALU round trip on every element).
// (m & x) | (~m & y) in one v_bfi_b32 (written out, the compiler turns it back into a compare
// into an SGPR mask + v_cndmask, with its s_nop hazard per element)
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t x, uint32_t y) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(x), "v"(y));
    return r;
}

__device__ __forceinline__ uint64_t keep_side(uint64_t a, uint64_t b, uint32_t flip) {
    const uint32_t m = (uint32_t)((int64_t)(a - b) >> 63) ^ flip;  // ~0: keep a
    return ((uint64_t)bfi(m, (uint32_t)(a >> 32), (uint32_t)(b >> 32)) << 32) | bfi(m, (uint32_t)a, (uint32_t)b);
}

__device__ __forceinline__ void cas_up(uint64_t& a, uint64_t& b) {
    const uint32_t m = (uint32_t)((int64_t)(a - b) >> 63);  // ~0: a < b
    const uint32_t ah = (uint32_t)(a >> 32), al = (uint32_t)a, bh = (uint32_t)(b >> 32), bl = (uint32_t)b;
    a = ((uint64_t)bfi(m, ah, bh) << 32) | bfi(m, al, bl);
    b = ((uint64_t)bfi(m, bh, ah) << 32) | bfi(m, bl, al);
}

// the same on 32-bit keys: one v_min_u32 + one v_max_u32
__device__ __forceinline__ void cas_up(uint32_t& a, uint32_t& b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

__device__ __forceinline__ uint32_t keep_side(uint32_t a, uint32_t b, uint32_t flip) {
    return bfi(flip, a > b ? a : b, a < b ? a : b);  // flip = ~0: max
}

// half cleaners of distance J, J / 2, .., 1
template <int E, int J, class K>
__device__ __forceinline__ void wave_half_cleaners(K (&v)[E], int lane) {
    if constexpr (J >= 1) {
        if constexpr (J >= E) {
            constexpr int L = J / E;
            const uint32_t flip = (lane & L) ? ~0u : 0u;
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = keep_side(v[e], lane_xor<L>(v[e]), flip);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((e & J) == 0) cas_up(v[e], v[e ^ J]);
        }
        wave_half_cleaners<E, J / 2>(v, lane);
    }
}

// merges of size K, 2K, .., 64 E
template <int E, int K, class T>
__device__ __forceinline__ void wave_bitonic(T (&v)[E], int lane) {
    if constexpr (K <= 64 * E) {
        if constexpr (K <= E) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((e & (K / 2)) == 0) cas_up(v[e], v[e ^ (K - 1)]);
        } else {
            // entry i = lane E + e pairs with i ^ (K - 1): lane ^ (K / E - 1), entry E - 1 - e
            constexpr int M = K / E - 1;
            const uint32_t flip = (lane & (K / (2 * E))) ? ~0u : 0u;
            if constexpr (E == 1) {
                v[0] = keep_side(v[0], lane_xor<M>(v[0]), flip);
            } else {
#pragma unroll
                for (int e = 0; e < E / 2; ++e) {
                    const T pa = lane_xor<M>(v[E - 1 - e]), pb = lane_xor<M>(v[e]);
                    v[e] = keep_side(v[e], pa, flip);
                    v[E - 1 - e] = keep_side(v[E - 1 - e], pb, flip);
                }
            }
        }
        wave_half_cleaners<E, K / 4>(v, lane);
        wave_bitonic<E, 2 * K>(v, lane);
    }
}

// index of word i in an LDS row padded by one word per 32 (a lane's E consecutive words and its
// neighbours' then fall in different banks)
__host__ __device__ constexpr int lds_pad(int i) { return i + (i >> 5); }

// the full (depth << 32 | gid) key of entry `pos` of the slice starting at `base`: from the placed
// (gid, key) pairs when there are any (src), else the gid and its gathered depth key
__device__ __forceinline__ uint64_t full_key(const uint2* __restrict__ src, const uint32_t* __restrict__ gid,
                                             const uint32_t* __restrict__ depth_key, uint32_t base, uint32_t pos) {
    if (src) {
        const uint2 p = src[base + pos];
        return ((uint64_t)p.y << 32) | p.x;
    }
    const uint32_t g = gid[base + pos];
    return ((uint64_t)depth_key[g] << 32) | g;
}

// The slice is read coalesced (entry e * 64 + lane into register e: the network sorts whatever
// order it is given) and, sorted (rank lane E + e in register e), written back through the wave's
// LDS rows so the stores are coalesced too (`xs`: 64 E + 64 E / 32 words, rows padded against bank
// conflicts).
template <int E>
__device__ __forceinline__ void wave_sort_slice(const uint2 rg, const uint32_t* __restrict__ depth_key,
                                                uint32_t* __restrict__ gid, int lane, uint32_t* xs,
                                                const uint2* __restrict__ src = nullptr) {
    const int n = (int)(rg.y - rg.x);
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        // padding sorts last (no real key reaches it)
        v[e] = i < n ? full_key(src, gid, depth_key, rg.x, i) : 0x7FFFFFFFFFFFFFFFull;
    }
    wave_bitonic<E, 2>(v, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) xs[lds_pad(lane * E + e)] = (uint32_t)v[e];
    wave_lds_sync();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        if (i < n) gid[rg.x + i] = xs[lds_pad(i)];
    }
    wave_lds_sync();  // xs reused by the wave's next slice
}

// ---- the same network on 32-bit keys (slices of <= 1024 entries) ----
// Key = the slice's top 22 differing depth bits over the entry's slice position (10 bits): half
// the cross-lane traffic of the 64-bit key (one DPP / swizzle / bpermute per exchange, not two)
// and a compare-exchange of one v_min_u32 + one v_max_u32.  Entries whose truncated depths are
// equal (the depth bits below the top 22 differing ones, or the whole depth, tie) come out in
// slice-position order; they are put in (depth, gid) order afterwards from the full keys -- in
// place by the lane holding a run's first entry when the run is short, else by the 64-bit form.
constexpr int kWaveKeyBits = 22, kWaveRunMax = 16;

// The truncated key of a slice whose depth keys have the or / and (kor, kand): the top KB bits
// among those in which the keys differ, over the entry's slice position in the 32 - KB bits below.
template <int KB>
struct TruncKey {
    int sh;
    __device__ __forceinline__ TruncKey(uint32_t kor, uint32_t kand) {
        const uint32_t dif = kor ^ kand;
        const int top = dif ? 32 - __clz(dif) : 0;  // differing bits [0, top)
        sh = top > KB ? top - KB : 0;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t dk, int pos) const {
        return (((dk >> sh) & ((1u << KB) - 1u)) << (32 - KB)) | (uint32_t)pos;
    }
};

template <int E>
__device__ __forceinline__ void wave_sort_slice32(const uint2 rg, const uint32_t* __restrict__ depth_key,
                                                  uint32_t* __restrict__ gid, int lane, uint32_t* xs,
                                                  const uint2* __restrict__ src = nullptr) {
    static_assert(64 * E <= (1 << (32 - kWaveKeyBits)), "slice position bits");
    constexpr uint32_t kPos = (1u << (32 - kWaveKeyBits)) - 1u;
    const int n = (int)(rg.y - rg.x);
    uint32_t v[E], dk[E];
    uint32_t kor = 0u, kand = ~0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        dk[e] = 0u;
        if (i < n) {
            dk[e] = src ? src[rg.x + i].y : depth_key[gid[rg.x + i]];
            kor |= dk[e];
            kand &= dk[e];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kor |= __shfl_xor(kor, o, 64);
        kand &= __shfl_xor(kand, o, 64);
    }
    const TruncKey<kWaveKeyBits> trunc(kor, kand);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        // padding ~0 sorts last: a real key reaches it only as the last of 1024 entries
        v[e] = i < n ? trunc(dk[e], i) : ~0u;
    }
    wave_bitonic<E, 2>(v, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) xs[lds_pad(lane * E + e)] = v[e];
    wave_lds_sync();
    // runs of equal truncated keys: the lane holding a run's first entry orders it by the full
    // (depth, gid) key (insertion; the slice's gids are still in place in gid[])
    auto full = [&](uint32_t x) { return full_key(src, gid, depth_key, rg.x, x & kPos); };
    bool tie = false, longrun = false;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int r = lane * E + e;
        if (r + 1 < n && (v[e] >> (32 - kWaveKeyBits)) == (xs[lds_pad(r + 1)] >> (32 - kWaveKeyBits))) tie = true;
    }
    if (__ballot(tie)) {  // wave-uniform; rare
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int r = lane * E + e;
            const uint32_t top_r = v[e] >> (32 - kWaveKeyBits);
            if (r + 1 >= n || (xs[lds_pad(r + 1)] >> (32 - kWaveKeyBits)) != top_r) continue;
            if (r > 0 && (xs[lds_pad(r - 1)] >> (32 - kWaveKeyBits)) == top_r) continue;  // not the run's first
            int end = r + 2;
            while (end < n && (xs[lds_pad(end)] >> (32 - kWaveKeyBits)) == top_r && end - r <= kWaveRunMax) ++end;
            if (end - r > kWaveRunMax) {
                longrun = true;
                continue;
            }
            for (int a = r + 1; a < end; ++a) {
                const uint32_t x = xs[lds_pad(a)];
                const uint64_t fx = full(x);
                int b = a;
                while (b > r && full(xs[lds_pad(b - 1)]) > fx) {
                    xs[lds_pad(b)] = xs[lds_pad(b - 1)];
                    --b;
                }
                xs[lds_pad(b)] = x;
            }
        }
        wave_lds_sync();
        if (__ballot(longrun)) {  // many entries at one truncated depth: the 64-bit form
            wave_sort_slice<E>(rg, depth_key, gid, lane, xs, src);
            return;
        }
    }
    // every read of the slice's gids completes before the first store over them (the compiler
    // would otherwise store each result as soon as its own load returned, while later loads of the
    // same slice were still in flight)
    uint32_t og[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        const uint32_t at = rg.x + (xs[lds_pad(i)] & kPos);
        og[e] = i < n ? (src ? src[at].x : gid[at]) : 0u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * 64 + lane;
        if (i < n) gid[rg.x + i] = og[e];
    }
    wave_lds_sync();  // xs reused by the wave's next slice
}

// Four tiles per 256-thread block, one per wave; slices longer than 1024 entries go to `ovf`.
__global__ __launch_bounds__(256) void tile_depth_wave(const uint2* __restrict__ ranges, int tile0, int ntiles,
                                                      const uint32_t* __restrict__ depth_key,
                                                      uint32_t* __restrict__ gid, uint32_t* __restrict__ ovf,
                                                      uint32_t* __restrict__ ovf_count,
                                                      const uint2* __restrict__ src) {
    __shared__ uint32_t xs_all[4][64 * 16 + 32];
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    const int lane = threadIdx.x & 63;
    uint32_t* const xs = xs_all[threadIdx.x >> 6];
    const int tile = tile0 + t;
    const uint2 rg = ranges[tile];
    const int n = (int)(rg.y - rg.x);
    if (n <= 1 || n > 1024) {
        // src: the later forms sort in place in gid[] -- the slice's gids go there first
        if (src)
            for (int i = lane; i < n; i += 64) gid[rg.x + i] = src[rg.x + i].x;
        if (n > 1 && lane == 0) ovf[atomicAdd(ovf_count, 1u)] = (uint32_t)tile;
        return;
    }
    if (n <= 64) wave_sort_slice32<1>(rg, depth_key, gid, lane, xs, src);
    else if (n <= 128) wave_sort_slice32<2>(rg, depth_key, gid, lane, xs, src);
    else if (n <= 256) wave_sort_slice32<4>(rg, depth_key, gid, lane, xs, src);
    else if (n <= 512) wave_sort_slice32<8>(rg, depth_key, gid, lane, xs, src);
    else wave_sort_slice32<16>(rg, depth_key, gid, lane, xs, src);
}

// The queued slices of 1025 .. 2048 entries, one wave each (a kernel of its own: the 32-entry-per-
// lane form needs ~230 VGPRs, which would cap the common form's occupancy at 2 waves per SIMD);
// longer ones go on to `ovf2` for the LDS form.  Launched only where the mean slice is near one
// wave's 1024 entries (multi-GPU bands at 1M: ~1060), where a good share of the slices exceed it;
// the queue length is on the device.
__global__ __launch_bounds__(256) void tile_depth_wave_queue(const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ depth_key,
                                                            uint32_t* __restrict__ gid,
                                                            const uint32_t* __restrict__ ovf,
                                                            const uint32_t* __restrict__ ovf_count,
                                                            uint32_t* __restrict__ ovf2,
                                                            uint32_t* __restrict__ ovf2_count) {
    __shared__ uint32_t xs_all[4][64 * 32 + 64];
    const uint32_t cnt = *ovf_count;
    const int lane = threadIdx.x & 63;
    uint32_t* const xs = xs_all[threadIdx.x >> 6];
    for (uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6); q < cnt; q += gridDim.x * 4) {
        const uint32_t tile = ovf[q];
        const uint2 rg = ranges[tile];
        const int n = (int)(rg.y - rg.x);
        if (n > 2048) {
            if (lane == 0) ovf2[atomicAdd(ovf2_count, 1u)] = tile;
            continue;  // wave-uniform
        }
        wave_sort_slice<32>(rg, depth_key, gid, lane, xs);
    }
}

// ---- per-tile depth order, block form: slices of 1025 .. NW x 1024 entries (round 6) ----
// Each of the block's NW waves sorts 1024 entries of the slice with the register network on
// 32-bit keys (the slice's top differing depth bits over the entry's slice position, as the
// one-wave form: 20 bits over 12 at 4096 entries, 19 over 13 at 8192); the waves' runs are then
// merged by the same all-ascending network, its stages at distances >= 1024 exchanged through LDS
// (one write, a barrier and one read per entry; padded rows: conflict-free) and the rest inside
// each wave: ~log2(n)^2 / 2 register stages, 3 (4096) or 6 (8192) LDS exchanges.  Runs of equal
// truncated keys are put in (depth, gid) order from the full keys by the thread holding a run's
// first entry; a run longer than kWaveRunMax (depths clustered inside one truncated step) leaves
// the slice untouched and hands the tile on (`false`) to the next queue, whose forms sort every bit.
// E: entries per lane (16: 1024 per wave)
constexpr int kBlkE = 16;
__host__ __device__ constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x >> 1); }
constexpr int kBlkW = 4096 / (64 * kBlkE), kBlkQW = 8192 / (64 * kBlkE);  // waves: <= 4096 / <= 8192
template <int NW>
struct BlockSortLds {
    uint32_t xs[lds_pad(NW * 64 * kBlkE)];
    uint32_t red[2][NW];
};

template <int NW>
__device__ __forceinline__ bool block_sort_slice(const uint2 rg, const uint32_t* __restrict__ depth_key,
                                                 uint32_t* __restrict__ gid, const uint2* __restrict__ src,
                                                 BlockSortLds<NW>& L) {
    constexpr int WE = 64 * kBlkE;  // entries per wave
    constexpr int CAP = NW * WE, NT = NW * 64;
    constexpr int PB = ilog2c(CAP);  // position bits
    constexpr int KB = 32 - PB;                           // truncated depth bits
    static_assert((1 << PB) == CAP, "position bits");
    constexpr uint32_t kPos = CAP - 1u;
    const int n = (int)(rg.y - rg.x);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    // active waves: the power of two whose runs cover the slice (the rest only meet the barriers)
    int nwa = 1;
    while (nwa * WE < n) nwa <<= 1;
    const bool act = w < nwa;
    uint32_t v[kBlkE];
    uint32_t kor = 0u, kand = ~0u;
#pragma unroll
    for (int e = 0; e < kBlkE; ++e) {
        const int i = w * WE + e * 64 + lane;
        v[e] = 0u;
        if (i < n) {
            v[e] = src ? src[rg.x + i].y : depth_key[gid[rg.x + i]];
            kor |= v[e];
            kand &= v[e];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kor |= __shfl_xor(kor, o, 64);
        kand &= __shfl_xor(kand, o, 64);
    }
    if (lane == 0) {
        L.red[0][w] = kor;
        L.red[1][w] = kand;
    }
    __syncthreads();
    {
        uint32_t o_ = 0u, a_ = ~0u;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            o_ |= L.red[0][k];
            a_ &= L.red[1][k];
        }
        kor = o_;
        kand = a_;
    }
    const TruncKey<KB> trunc(kor, kand);
#pragma unroll
    for (int e = 0; e < kBlkE; ++e) {
        const int i = w * WE + e * 64 + lane;
        // padding ~0 sorts last: a real key reaches it only at position CAP - 1, i.e. n = CAP
        v[e] = i < n ? trunc(v[e], i) : ~0u;
    }
    if (act) wave_bitonic<kBlkE, 2>(v, lane);  // each active wave's WE entries, ascending
    // merges of the waves' runs: entry i = w WE + E lane + e
    const int i0 = w * WE + lane * kBlkE;
    uint32_t* const xs = L.xs;
    auto lds_stage = [&](int x, int h) {  // i <-> i ^ x, the lower of the pair (i & h == 0) keeps the min
        if (act) {
#pragma unroll
            for (int e = 0; e < kBlkE; ++e) xs[lds_pad(i0 + e)] = v[e];
        }
        __syncthreads();
        if (act) {
            const bool hi = (i0 & h) != 0;  // the same for the lane's E entries (h >= WE)
#pragma unroll
            for (int e = 0; e < kBlkE; ++e) {
                const uint32_t o = xs[lds_pad((i0 + e) ^ x)];
                v[e] = hi ? (v[e] > o ? v[e] : o) : (v[e] < o ? v[e] : o);
            }
        }
        __syncthreads();  // xs is rewritten by the next stage
    };
    for (int K = 2 * WE; K <= nwa * WE; K <<= 1) {  // block-uniform
        lds_stage(K - 1, K >> 1);                     // the mirror stage
        for (int J = K >> 2; J >= WE; J >>= 1) lds_stage(J, J);
        if (act) wave_half_cleaners<kBlkE, WE / 2>(v, lane);
    }
    // the sorted keys by rank, then the runs of equal truncated keys
    if (act) {
#pragma unroll
        for (int e = 0; e < kBlkE; ++e) xs[lds_pad(i0 + e)] = v[e];
    }
    __syncthreads();
    bool tie = false;
    if (act) {
#pragma unroll
        for (int e = 0; e < kBlkE; ++e) {
            const int r = i0 + e;
            if (r + 1 < n && (v[e] >> PB) == (xs[lds_pad(r + 1)] >> PB)) tie = true;
        }
    }
    if (__syncthreads_or(tie)) {  // block-uniform
        auto full = [&](uint32_t x) { return full_key(src, gid, depth_key, rg.x, x & kPos); };
        bool longrun = false;
        if (act) {
#pragma unroll
            for (int e = 0; e < kBlkE; ++e) {
                const int r = i0 + e;
                const uint32_t top_r = v[e] >> PB;
                if (r + 1 >= n || (xs[lds_pad(r + 1)] >> PB) != top_r) continue;
                if (r > 0 && (xs[lds_pad(r - 1)] >> PB) == top_r) continue;  // not the run's first
                int end = r + 2;
                while (end < n && (xs[lds_pad(end)] >> PB) == top_r && end - r <= kWaveRunMax) ++end;
                if (end - r > kWaveRunMax) {
                    longrun = true;
                    continue;
                }
                if (end - r <= 4) {
                    // the common run (2 - 3 entries at 5M / 1080p): its full keys loaded together --
                    // one global round trip, not one per insertion step -- and a 4-entry network
                    uint32_t xx[4];
                    uint64_t fk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool in = r + j < end;
                        xx[j] = in ? xs[lds_pad(r + j)] : 0u;
                        fk[j] = in ? full(xx[j]) : ~0ull;
                    }
                    auto cx = [&](int a, int b) {
                        if (fk[b] < fk[a]) {
                            const uint64_t t = fk[a];
                            fk[a] = fk[b];
                            fk[b] = t;
                            const uint32_t u = xx[a];
                            xx[a] = xx[b];
                            xx[b] = u;
                        }
                    };
                    cx(0, 1);
                    cx(2, 3);
                    cx(0, 2);
                    cx(1, 3);
                    cx(1, 2);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (r + j < end) xs[lds_pad(r + j)] = xx[j];
                    continue;
                }
                for (int a = r + 1; a < end; ++a) {  // insertion by the full (depth, gid) key
                    const uint32_t x = xs[lds_pad(a)];
                    const uint64_t fx = full(x);
                    int b = a;
                    while (b > r && full(xs[lds_pad(b - 1)]) > fx) {
                        xs[lds_pad(b)] = xs[lds_pad(b - 1)];
                        --b;
                    }
                    xs[lds_pad(b)] = x;
                }
            }
        }
        if (__syncthreads_or(longrun)) return false;  // nothing written: the next form sorts it
    }
    // out in rank order (in place without src: every thread's reads of the slice's gids complete,
    // block-wide, before the first store over them)
    uint32_t og[CAP / NT];
#pragma unroll
    for (int k = 0; k < CAP / NT; ++k) {
        const int r = k * NT + tid;
        const uint32_t at = rg.x + (xs[lds_pad(r < n ? r : 0)] & kPos);
        og[k] = r < n ? (src ? src[at].x : gid[at]) : 0u;
    }
    if (!src) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < CAP / NT; ++k) {
        const int r = k * NT + tid;
        if (r < n) gid[rg.x + r] = og[k];
    }
    __syncthreads();  // xs / red are rewritten by the block's next slice
    return true;
}

// launches of fewer tiles (multi-GPU bands) sort every deep slice with the 8-wave form in one round
#ifndef GSR_BLOCK8_TILES
#define GSR_BLOCK8_TILES 4096
#endif

// One block of NW waves per tile of the launch (slices of up to NW x 1024 entries); longer slices,
// and those with long runs of equal truncated keys, go to `ovf`: NW = 4 (full images) hands them to
// the 8-wave queue below, which reads src too; NW = 8 (band launches, ~1000 tiles: one round of
// blocks instead of two, the first one's 4096-entry sorts and then the queued longer ones) hands
// them to tile_depth_sort_big, which sorts in place -- their gids are copied to gid[] first.
template <int NW>
__global__ __launch_bounds__(NW * 64) void tile_depth_block(const uint2* __restrict__ ranges, int tile0,
                                                           const uint32_t* __restrict__ depth_key,
                                                           uint32_t* __restrict__ gid, uint32_t* __restrict__ ovf,
                                                           uint32_t* __restrict__ ovf_count,
                                                           const uint2* __restrict__ src) {
    __shared__ BlockSortLds<NW> lds;
    const int tile = tile0 + blockIdx.x;
    const uint2 rg = ranges[tile];
    const int n = (int)(rg.y - rg.x);
    if (n <= 1) {
        if (n == 1 && src && threadIdx.x == 0) gid[rg.x] = src[rg.x].x;
        return;
    }
    if (n > NW * 64 * kBlkE || !block_sort_slice<NW>(rg, depth_key, gid, src, lds)) {  // block-uniform
        if (NW == kBlkQW && src)
            for (int i = threadIdx.x; i < n; i += NW * 64) gid[rg.x + i] = src[rg.x + i].x;
        if (threadIdx.x == 0) ovf[atomicAdd(ovf_count, 1u)] = (uint32_t)tile;
    }
}

// The queued slices of up to 8192 entries, eight waves per block, one queued tile per block (the
// grid covers every tile; blocks past the queue's length exit at once); longer ones and those with
// long truncated-key runs go on to `ovf2` (tile_depth_sort_big sorts every bit).
__global__ __launch_bounds__(64 * kBlkQW) void tile_depth_block_queue(const uint2* __restrict__ ranges,
                                                             const uint32_t* __restrict__ depth_key,
                                                             uint32_t* __restrict__ gid,
                                                             const uint32_t* __restrict__ ovf,
                                                             const uint32_t* __restrict__ ovf_count,
                                                             uint32_t* __restrict__ ovf2,
                                                             uint32_t* __restrict__ ovf2_count,
                                                             const uint2* __restrict__ src) {
    __shared__ BlockSortLds<kBlkQW> lds;
    if (blockIdx.x >= *ovf_count) return;
    const uint32_t tile = ovf[blockIdx.x];
    const uint2 rg = ranges[tile];
    const int n = (int)(rg.y - rg.x);
    if (n > 8192 || !block_sort_slice<kBlkQW>(rg, depth_key, gid, src, lds)) {  // block-uniform
        // tile_depth_sort_big sorts in place in gid[]: the slice's gids go there first
        if (src)
            for (int i = threadIdx.x; i < n; i += 64 * kBlkQW) gid[rg.x + i] = src[rg.x + i].x;
        if (threadIdx.x == 0) ovf2[atomicAdd(ovf2_count, 1u)] = tile;
    }
}

// Slices of 8193 and more entries (dense tiles of training views): one kernel, 1024-thread
// blocks, 8 work items per queued tile.  A slice of <= 16384 entries is sorted whole in LDS by
// item 0 (~145 KB: gfx950 gives one workgroup up to 160 KiB).  A longer slice is cut into
// 16384-entry chunks, sorted in place by the tile's items in parallel (a chunk is in gid order,
// so the stable depth sort leaves it in (depth, gid) order), and the item that finishes last
// (a per-tile counter, device-scope fences on both sides) merges them: the rest of an
// all-ascending ("flip") bitonic network over the range padded to a power of two, whose stages
// through size 16384 the sorted chunks already satisfy.  Strides >= 16384 run in global memory
// on the 64-bit (depth << 32 | gid) key split over two u32 arrays (the tile sort's free
// ping-pong pair); shorter strides in LDS one chunk at a time.  A 40k-entry tile takes 3 global
// passes and 2 x 3 LDS chunk passes instead of the 136 global passes of a plain bitonic sort.
constexpr int kBigChunk = 16384;
static_assert(kBigChunk == kSliceNT * kSliceI, "a chunk is one slice sort");
static_assert(sizeof(SliceLds) >= kBigChunk * sizeof(uint64_t), "merge chunk aliases the slice LDS");

// One bitonic half-cleaner stage (pairs i <-> i + d) over the LDS chunk.  The chunk is padded
// with ~0 sentinels, which no real (depth, gid) pair reaches (gid < 2^32-1).
__device__ __forceinline__ void lds_half_cleaner(uint64_t* sk, int d) {
    for (int t = threadIdx.x; t < kBigChunk / 2; t += 1024) {
        const int i = ((t & ~(d - 1)) << 1) | (t & (d - 1));
        const uint64_t a = sk[i], b = sk[i + d];
        if (a > b) sk[i] = b, sk[i + d] = a;
    }
    __syncthreads();
}

// The big form's LDS: the slice sort's arrays, or the merge's 16384 packed keys.  At namespace
// scope so that the two out-of-line phases below address it as LDS directly; each has the
// 128-VGPR budget of a 1024-thread block to itself (inlined into one loop nest, the slice
// sort's 48 key / value / rank registers spilled).
__shared__ union BigLds {
    SliceLds slice;
    uint64_t sk[kBigChunk];
} g_big;

__device__ __attribute__((noinline)) void big_slice_sort(const uint2 rg, const uint32_t* __restrict__ depth_key,
                                                         uint32_t* __restrict__ gid, bool unordered) {
    radix_sort_slice(rg, depth_key, gid, g_big.slice, unordered);
}

__device__ __attribute__((noinline)) void merge_sorted_chunks(const uint2 r, const uint32_t* __restrict__ depth_key,
                                                              uint32_t* __restrict__ gid, uint32_t* __restrict__ hi,
                                                              uint32_t* __restrict__ lo) {
    uint64_t* const sk = g_big.sk;
    const int n = (int)(r.y - r.x);
    int m = kBigChunk;
    while (m < n) m <<= 1;
    const int nch = (n + kBigChunk - 1) / kBigChunk;
    uint32_t* H = hi + r.x;
    uint32_t* L = lo + r.x;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const uint32_t g = gid[r.x + i];
        H[i] = depth_key[g];
        L[i] = g;
    }
    __syncthreads();
    auto cex = [&](int i, int j) {  // i < j; indices >= n are +inf padding
        if (j >= n) return;
        const uint64_t a = ((uint64_t)H[i] << 32) | L[i], b = ((uint64_t)H[j] << 32) | L[j];
        if (a > b) {
            H[i] = (uint32_t)(b >> 32), L[i] = (uint32_t)b;
            H[j] = (uint32_t)(a >> 32), L[j] = (uint32_t)a;
        }
    };
    for (int size = 2 * kBigChunk; size <= m; size <<= 1) {
        for (int d = size >> 1; d >= kBigChunk; d >>= 1) {
            const bool flip = d == (size >> 1);
            for (int t = threadIdx.x; t < (m >> 1); t += 1024) {
                const int i = ((t & ~(d - 1)) << 1) | (t & (d - 1));
                cex(i, flip ? (i ^ (size - 1)) : (i + d));
            }
            __syncthreads();
        }
        const bool last = size == m;
        for (int c = 0; c < nch; ++c) {
            const int base = c * kBigChunk;
            for (int i = threadIdx.x; i < kBigChunk; i += 1024)
                sk[i] = base + i < n ? (((uint64_t)H[base + i] << 32) | L[base + i]) : ~0ull;
            __syncthreads();
            for (int d = kBigChunk >> 1; d >= 1; d >>= 1) lds_half_cleaner(sk, d);
            for (int i = threadIdx.x; i < kBigChunk && base + i < n; i += 1024) {
                const uint64_t v = sk[i];
                if (last) {
                    gid[r.x + base + i] = (uint32_t)v;
                } else {
                    H[base + i] = (uint32_t)(v >> 32);
                    L[base + i] = (uint32_t)v;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(1024) void tile_depth_sort_big(const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ depth_key,
                                                            uint32_t* __restrict__ gid,
                                                            const uint32_t* __restrict__ ovf,
                                                            const uint32_t* __restrict__ ovf_count,
                                                            uint32_t* __restrict__ done,
                                                            uint32_t* __restrict__ hi, uint32_t* __restrict__ lo,
                                                            int unordered) {
    __shared__ uint32_t last;
    const uint32_t cnt = *ovf_count;
    // item-major: the first cnt work items are every tile's item 0, spread over all blocks
    for (uint32_t w = blockIdx.x; w < 8u * cnt; w += gridDim.x) {
        const uint32_t q = w % cnt, item = w / cnt;
        const uint2 r = ranges[ovf[q]];
        const uint32_t n = r.y - r.x;
        // a slice of <= kBigChunk entries is item 0's whole; a longer one is cut into chunks
        const bool whole = n <= (uint32_t)kBigChunk;
        const uint32_t nch = whole ? 1u : (n + kBigChunk - 1) / kBigChunk;
        const uint32_t parts = nch < 8u ? nch : 8u;
        if (item >= parts) continue;  // block-uniform
        for (uint32_t c0 = r.x + item * kBigChunk; c0 < r.y; c0 += 8u * kBigChunk) {
            const uint32_t c1 = whole || c0 + kBigChunk >= r.y ? r.y : c0 + kBigChunk;
            big_slice_sort(make_uint2(c0, c1), depth_key, gid, unordered != 0);
        }
        if (whole) continue;
        __threadfence();  // this item's chunks visible device-wide before it counts itself done
        __syncthreads();
        if (threadIdx.x == 0) last = atomicAdd(done + q, 1u) == parts - 1u ? 1u : 0u;
        __syncthreads();
        if (!last) continue;  // block-uniform
        __threadfence();      // acquire: the other items' chunks
        merge_sorted_chunks(r, depth_key, gid, hi, lo);
    }
}

}  // namespace

// the slice capacity the per-tile sort picks for a mean slice of K / ntiles entries
static int tile_sort_cap(long long K, int ntiles) {
    const long long mean = ntiles > 0 ? K / ntiles : K;
    int cap = 1024;
    while (cap < 4096 && cap < mean + mean / 2) cap <<= 1;
    return cap;
}

int launch_tile_depth_sort(const uint2* ranges, int tile0, int ntiles, long long K, const uint32_t* depth_key,
                           uint32_t* gid, uint32_t* ovf, uint32_t* ovf_count, uint32_t* ovf2, uint32_t* ovf2_count,
                           uint32_t* done, uint32_t* scratch_hi, uint32_t* scratch_lo, hipStream_t s,
                           bool unordered, const uint2* src) {
    if (ntiles <= 0 || K <= 0) return 0;
    const int uo = unordered ? 1 : 0;
    const int bgrid = ntiles < 256 ? ntiles : 256;  // tile_depth_sort_big's blocks walk its queue
    // Mean slices of up to ~1365 entries (cap <= 2048): slices of up to 1024 entries sorted in
    // registers, one wave each (the mean leaves most tiles within that).
    if (tile_sort_cap(K, ntiles) <= 2048) {
        hipLaunchKernelGGL(tile_depth_wave, dim3(div_up(ntiles, 4)), dim3(256), 0, s, ranges, tile0, ntiles, depth_key,
                           gid, ovf, ovf_count, src);
        // the slices past one wave's 1024 entries: where the mean is near 1024 (bands), many -- a
        // 2048-entry wave each, the rest on to the LDS form; elsewhere few (none at 1M / 1080p) --
        // all straight to the 1024-thread LDS form, one launch instead of two more near-empty
        // ones (~5 us each)
        if (K / ntiles > 900) {
            const int wgrid = ntiles < 2048 ? div_up(ntiles, 4) : 512;
            hipLaunchKernelGGL(tile_depth_wave_queue, dim3(wgrid), dim3(256), 0, s, ranges, depth_key, gid, ovf,
                               ovf_count, ovf2, ovf2_count);
            hipLaunchKernelGGL(tile_depth_sort_big, dim3(bgrid), dim3(1024), 0, s, ranges, depth_key, gid, ovf2,
                               ovf2_count, done, scratch_hi, scratch_lo, uo);
        } else {
            hipLaunchKernelGGL(tile_depth_sort_big, dim3(bgrid), dim3(1024), 0, s, ranges, depth_key, gid, ovf,
                               ovf_count, done, scratch_hi, scratch_lo, uo);
        }
    } else if (ntiles < GSR_BLOCK8_TILES) {  // deep slices, few tiles (bands): 8 waves per tile, one round
        hipLaunchKernelGGL(tile_depth_block<kBlkQW>, dim3(ntiles), dim3(64 * kBlkQW), 0, s, ranges, tile0, depth_key, gid, ovf2,
                           ovf2_count, src);
        hipLaunchKernelGGL(tile_depth_sort_big, dim3(bgrid), dim3(1024), 0, s, ranges, depth_key, gid, ovf2,
                           ovf2_count, done, scratch_hi, scratch_lo, uo);
    } else {  // deep slices: the 4-wave block form, then its 8192-entry queue
        // (one 8192-entry block per tile at 5M / 1080p: 0.89 ms with 512 threads, 0.79 with 1024,
        // against 0.49 for 4096-entry blocks + the queue: 1 block per CU)
        hipLaunchKernelGGL(tile_depth_block<kBlkW>, dim3(ntiles), dim3(64 * kBlkW), 0, s, ranges, tile0, depth_key, gid, ovf,
                           ovf_count, src);
        hipLaunchKernelGGL(tile_depth_block_queue, dim3(ntiles), dim3(64 * kBlkQW), 0, s, ranges, depth_key, gid, ovf,
                           ovf_count, ovf2, ovf2_count, src);
        hipLaunchKernelGGL(tile_depth_sort_big, dim3(bgrid), dim3(1024), 0, s, ranges, depth_key, gid, ovf2,
                           ovf2_count, done, scratch_hi, scratch_lo, uo);
    }
    return (int)hipGetLastError();
}

}  // namespace gsr
