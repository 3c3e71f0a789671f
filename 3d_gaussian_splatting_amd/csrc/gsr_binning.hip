// gsr_binning.hip -- binning on gfx950: the scan of tiles_touched (F2), duplicateWithKeys (F3), the
// presort's rank-order payload, the row-bucketed binning, and the tile ranges (F5).
//
// Canonical instance order is (tile, depth bits, gid) (SURVEY §8a notes).  It is reached with far
// fewer sorted bytes than one 45-bit key sort over K instances, on one of three paths (gsr_api.cpp
// picks: use_presort / use_rb_binning in gsr_internal.h):
//   - scan + duplicate + radix: an inclusive scan of tiles_touched in gid order (offsets; K = the
//     last; one look-back kernel fused with the emission up to kFusedScanMax Gaussians, three scan
//     kernels above); Gaussian g emits its band-clipped rect row-major at offsets[g - 1]; a stable
//     LSD sort over the ceil(log2 tiles)-bit tile key only (gsr_radix.hip) groups the instances by
//     tile, gid order inside; finalize_kernel writes the ranges from the key boundaries; the
//     per-tile depth order (gsr_tilesort.hip) sorts each slice.
//   - presort: the P depth keys sorted first (gsr_radix.hip), each rank's (tiles, rect, gid)
//     gathered into rank order (rank_payload_kernel), scan + emission in rank order
//     (duplicate_kernel<true>); the stable tile-key sort leaves every tile in (depth, gid) order.
//   - row-bucketed (the rb_* kernels): F3, the tile sort and F5 as two counting passes over
//     (Gaussian, tile row) pairs; a tile's entries come out contiguous but unordered, and the
//     per-tile depth order sorts them by the whole (depth, gid) key.
// (B1 recovers an instance's emission index j from its Gaussian's rect, so no permutation array
// is carried through any of them.)
//
// K never has to reach the host: the scan writes it to a device word (total_out), and every
// later stage is launched for the binning's capacity and reads the live count from that word
// (instances past the capacity are dropped -- an overflow the caller detects from K).
#include "gsr_kernels.h"
#include "gsr_sort_dev.h"

namespace gsr {
namespace {

constexpr int kB = kSortBlock;  // 256 threads = 4 waves
constexpr int kI = kSortItems;  // 16 items per thread
constexpr int kWaves = kB / 64;

// ---- F2 scan of tiles_touched (gid order): reduce / partial scan / downsweep ----
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    const int nw = blockDim.x >> 6;
    for (int k = 0; k < nw; ++k) {
        pre += (k < w) ? wsum[k] : 0u;
        tot += wsum[k];
    }
    __syncthreads();
    *total = tot;
    return pre + x - v;
}

__global__ __launch_bounds__(kB) void scan_reduce(const uint32_t* __restrict__ in, int n,
                                                  uint32_t* __restrict__ partials) {
    __shared__ uint32_t wsum[kWaves];
    const int base = blockIdx.x * kSortTile;
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < kI; ++r) {
        const int i = base + r * kB + threadIdx.x;
        if (i < n) s += in[i];
    }
    uint32_t tot;
    block_exclusive_scan(s, wsum, &tot);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// Exclusive scan of n words in place by one block of 1024 threads, kScanQ contiguous words per
// thread per round (all of a round's loads issued before its block scan): one load latency and
// one block scan per 8192 words, not per 1024.  The form for rows past kScanQ1 x 1024 words;
// shorter rows take wide_block_scan_lds.
constexpr int kScanQ = 8, kScanQ1 = 32;
__device__ __forceinline__ uint32_t wide_block_scan(uint32_t* __restrict__ a, int n, uint32_t* wsum) {
    uint32_t carry = 0;
    for (int base = 0; base < n; base += 1024 * kScanQ) {
        const int i0 = base + (int)threadIdx.x * kScanQ;
        uint32_t v[kScanQ], sv = 0;
#pragma unroll
        for (int q = 0; q < kScanQ; ++q) {
            v[q] = i0 + q < n ? a[i0 + q] : 0u;
            sv += v[q];
        }
        uint32_t tot;
        uint32_t run = carry + block_exclusive_scan(sv, wsum, &tot);
#pragma unroll
        for (int q = 0; q < kScanQ; ++q) {
            if (i0 + q < n) a[i0 + q] = run;
            run += v[q];
        }
        carry += tot;
    }
    return carry;
}

// Up to kScanQ1 x 1024 words (the F2 block sums at 5M: 19.5k) in one round through LDS (dynamic
// LDS of n words): Q = ceil(n / 1024) consecutive words per thread, one load latency, one block
// scan, one store pass (three serial rounds of 8192 took ~7 us each at 5M).  The array is loaded
// and stored coalesced (word i by thread i mod 1024), and each thread scans its Q consecutive
// words out of LDS -- loads of Q consecutive words per thread straight from memory touch a
// different cache line in every lane of every load instruction.
__device__ __forceinline__ uint32_t wide_block_scan_lds(uint32_t* __restrict__ a, int n, uint32_t* wsum,
                                                        uint32_t* buf) {
    for (int i = (int)threadIdx.x; i < n; i += 1024) buf[i] = a[i];
    __syncthreads();
    const int Q = (n + 1023) / 1024;
    const int i0 = (int)threadIdx.x * Q;
    uint32_t v[kScanQ1], sv = 0;
#pragma unroll
    for (int q = 0; q < kScanQ1; ++q) {
        v[q] = q < Q && i0 + q < n ? buf[i0 + q] : 0u;
        sv += v[q];
    }
    uint32_t tot;
    uint32_t run = block_exclusive_scan(sv, wsum, &tot);
#pragma unroll
    for (int q = 0; q < kScanQ1; ++q) {
        if (q < Q && i0 + q < n) buf[i0 + q] = run;
        run += v[q];
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < n; i += 1024) a[i] = buf[i];
    return tot;
}
__host__ __device__ constexpr bool scan_lds_fits(long long n) { return n <= 1024LL * kScanQ1; }

// exclusive scan of the nb block totals in place; the grand total to *total_out
__global__ __launch_bounds__(1024) void scan_partials(uint32_t* __restrict__ partials, int nb,
                                                      uint32_t* __restrict__ total_out) {
    extern __shared__ uint32_t sbuf[];
    __shared__ uint32_t wsum[16];
    const uint32_t carry = scan_lds_fits(nb) ? wide_block_scan_lds(partials, nb, wsum, sbuf)
                                             : wide_block_scan(partials, nb, wsum);
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

// the row-bucketed binning's column scan: row r's per-block pair counts (histA[r][*]) in place,
// the row total to totA[r]; one 1024-thread block per row
__global__ __launch_bounds__(1024) void rb_colscan(uint32_t* __restrict__ hist, int nb, uint32_t* __restrict__ totals) {
    extern __shared__ uint32_t sbuf[];
    __shared__ uint32_t wsum[16];
    uint32_t* const a = hist + (size_t)blockIdx.x * nb;
    const uint32_t carry = scan_lds_fits(nb) ? wide_block_scan_lds(a, nb, wsum, sbuf) : wide_block_scan(a, nb, wsum);
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
static size_t scan_lds_bytes(long long n) { return scan_lds_fits(n) ? sizeof(uint32_t) * (size_t)n : 0; }

__global__ __launch_bounds__(kB) void scan_downsweep(const uint32_t* __restrict__ in, int n,
                                                     const uint32_t* __restrict__ partials,
                                                     uint32_t* __restrict__ out) {
    __shared__ uint32_t buf[kSortTile + kSortTile / 32];
    __shared__ uint32_t wsum[kWaves];
    const int base = blockIdx.x * kSortTile;
    const int tid = threadIdx.x;
    auto pad = [](int i) { return i + (i >> 5); };
#pragma unroll
    for (int r = 0; r < kI; ++r) {
        const int i = r * kB + tid;
        const int g = base + i;
        buf[pad(i)] = g < n ? in[g] : 0u;
    }
    __syncthreads();
    uint32_t v[kI];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kI; ++k) {
        v[k] = buf[pad(tid * kI + k)];
        s += v[k];
        v[k] = s;  // thread-local inclusive
    }
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(s, wsum, &tot) + partials[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kI; ++k) buf[pad(tid * kI + k)] = v[k] + ex;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kI; ++r) {
        const int i = r * kB + tid;
        if (base + i < n) out[base + i] = buf[pad(i)];
    }
}

// ---- F3 duplicate: wave-cooperative expansion (one wave = 64 consecutive Gaussians, whose
// instances are contiguous; lanes write consecutive instances -> coalesced stores) ----
__device__ __forceinline__ uint32_t udiv_small(uint32_t a, uint32_t b) {
    // a / b for a < 2^20, 1 <= b < 2^12: the float quotient of (a + 0.5) is at least 0.5 / b
    // away from an integer and rcp is accurate to ~1 ulp, so truncation is exact
    return (uint32_t)(((float)a + 0.5f) * __builtin_amdgcn_rcpf((float)b));
}

// Emission of one wave's instances [first, first + wtotal): lane i finds its owner -- the last
// lane whose start (s_start, relative to `first`) is <= i -- by binary search in LDS and writes
// (tile key, gid).  Instances at or past `cap` are dropped (binning overflow).
__device__ __forceinline__ void emit_wave(const uint32_t* s_start, const uint32_t* s_g, const uint32_t* s_w,
                                          const uint32_t* s_x0, const uint32_t* s_y0, uint32_t first,
                                          uint32_t wtotal, int grid_x, long long cap, uint32_t* __restrict__ tkey,
                                          uint32_t* __restrict__ tgid) {
    const int lane = threadIdx.x & 63;
    for (uint32_t i = lane; i < wtotal; i += 64) {
        if ((long long)first + i >= cap) break;
        int o = 0;  // lanes without instances never own one (their start is 0xFFFFFFFF)
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            if (s_start[o + step] <= i) o += step;
        const uint32_t local = i - s_start[o];
        const uint32_t wd = s_w[o];
        const uint32_t dy = udiv_small(local, wd), dx = local - dy * wd;
        tkey[first + i] = (s_y0[o] + dy) * (uint32_t)grid_x + s_x0[o] + dx;
        tgid[first + i] = s_g[o];
    }
}

// ---- fused F2 + F3: scan of tiles_touched in gid order + duplicate, one kernel ----
// Block b (in launch order, atomic ticket) owns Gaussians [256 b, 256 b + 256): it scans their
// tiles_touched, finds the instances of all earlier blocks by a wave-parallel decoupled
// look-back (64 predecessors per probe; relaxed agent-scope atomics on packed flag|count
// words), writes offsets / inst_start, and emits its own instances exactly as
// duplicate_kernel does.  Replaces three scan kernels + a second pass over the Gaussians; shipped
// for n <= 2^19 (a full 1M scene's look-back chain over n / 256 blocks costs more than the
// three-kernel scan: 0.102 vs 0.084 ms).
constexpr uint32_t kAgg = 1u << 30, kInc = 2u << 30, kCntMask = kAgg - 1u;

__global__ __launch_bounds__(256) void scan_duplicate_kernel(const uint32_t* __restrict__ tiles,
                                                             uint4* __restrict__ rect, int n,
                                                             int grid_x, int ty0,
                                                             uint32_t* __restrict__ offsets,
                                                             uint32_t* __restrict__ tkey,
                                                             uint32_t* __restrict__ tgid, long long cap,
                                                             uint32_t* __restrict__ status,
                                                             uint32_t* __restrict__ ticket,
                                                             uint32_t* __restrict__ total_out) {
    __shared__ uint32_t s_start[kWaves][64], s_g[kWaves][64], s_w[kWaves][64], s_x0[kWaves][64],
        s_y0[kWaves][64];
    __shared__ uint32_t wsum[kWaves];
    __shared__ uint32_t s_excl;
    __shared__ int s_b;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (tid == 0) s_b = (int)atomicAdd(ticket, 1u);
    __syncthreads();
    const int b = s_b;
    const int g = b * 256 + tid;
    const bool valid = g < n;
    uint32_t nt = 0, minx = 0, maxx = 0, y0 = 0;
    if (valid) {
        nt = tiles[g];
        if (nt) {
            const uint4 rr = rect[g];
            minx = rr.x & 0xFFFF;
            maxx = rr.y & 0xFFFF;
            const uint32_t miny = rr.x >> 16;
            y0 = miny > (uint32_t)ty0 ? miny : (uint32_t)ty0;
        }
    }
    // block scan
    uint32_t x = nt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        pre += (k < w) ? wsum[k] : 0u;
        total += wsum[k];
    }
    // look-back (wave 0)
    if (w == 0) {
        uint32_t excl = 0;
        if (b == 0) {
            if (lane == 0) __hip_atomic_store(status, kInc | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(status + b, kAgg | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int pos = b - 1;
            uint32_t spins = 0;
            while (true) {
                const int idx = pos - lane;
                uint32_t v = kInc;  // before block 0: an inclusive zero
                if (idx >= 0) v = __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (__ballot((v & ~kCntMask) == 0u)) {  // some predecessor not published yet
                    if (++spins > (1u << 24)) break;     // never expected; bounded so a bug cannot hang
                    __builtin_amdgcn_s_sleep(1);
                    if (idx >= 0 && (v & ~kCntMask) == 0u)
                        v = __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const uint64_t inc = __ballot((v & kInc) != 0u);
                const int k = inc ? __builtin_ctzll(inc) : 64;  // nearest inclusive predecessor
                uint32_t c = lane <= k ? (v & kCntMask) : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
                excl += c;
                if (inc || spins > (1u << 24)) break;
                pos -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(status + b, kInc | (excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_excl = excl;
    }
    __syncthreads();
    const uint32_t excl = s_excl;
    const uint32_t lex = pre + x - nt;  // block-local exclusive offset
    if (valid) {
        offsets[g] = excl + lex + nt;
        if (nt) rect[g].z = excl + lex;  // inst_start
    }
    if (total_out && tid == 0 && (b + 1) * 256 >= n) *total_out = excl + total;  // the last block: K
    // emission: this wave's instances [excl + pre_w, + wsum[w]) with pre_w = first lane's lex
    const uint32_t wbase = pre;  // = lex of lane 0 of this wave
    // the owner search needs starts non-decreasing across the wave: a Gaussian without tiles
    // keeps its (shared) start and never owns an instance; lanes past n sort last
    s_start[w][lane] = valid ? lex - wbase : 0xFFFFFFFFu;
    s_g[w][lane] = (uint32_t)g;
    s_w[w][lane] = maxx - minx;
    s_x0[w][lane] = minx;
    s_y0[w][lane] = y0;
    wave_lds_sync();
    emit_wave(s_start[w], s_g[w], s_w[w], s_x0[w], s_y0[w], excl + wbase, wsum[w], grid_x, cap, tkey, tgid);
}

// RANKED (presort mode): lane i is depth rank i; its tiles / rect / gid come from the rank-order
// payload (rtiles / rrect, coalesced) and inst_start goes to rect[gid] (one scattered word).
// RANKED also scans: `bexcl` holds the exclusive offsets of the 256-rank blocks (rank_payload_kernel
// summed each block, scan_partials scanned the sums), the block scans its own ranks and writes
// `offsets` (the gather reads them) -- the three-kernel scan's reduce and downsweep passes gone.
template <bool RANKED>
__global__ __launch_bounds__(256) void duplicate_kernel(uint32_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ tiles,
                                                        uint4* __restrict__ rect, const uint4* __restrict__ rrect,
                                                        int P, int grid_x, int ty0,
                                                        uint32_t* __restrict__ tkey, uint32_t* __restrict__ tgid,
                                                        long long cap, const uint32_t* __restrict__ bexcl) {
    __shared__ uint32_t s_start[kWaves][64], s_g[kWaves][64], s_w[kWaves][64], s_x0[kWaves][64],
        s_y0[kWaves][64];
    __shared__ uint32_t wsum[kWaves];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x * 256 + tid;  // gid, or depth rank (RANKED)
    const bool valid = i < P;
    uint32_t nt = 0, end = 0, g = (uint32_t)i;
    if (RANKED) {
        if (valid) nt = tiles[i];
        uint32_t tot;
        end = bexcl[blockIdx.x] + block_exclusive_scan(nt, wsum, &tot) + nt;
        if (valid) offsets[i] = end;
    } else if (valid) {
        nt = tiles[i];
        end = offsets[i];
    }
    uint32_t minx = 0, maxx = 0, y0 = 0;
    if (nt) {
        uint4 rr;
        if (RANKED) {
            rr = rrect[i];
            g = rr.z;
            rect[g].z = end - nt;  // inst_start
        } else {
            rect[g].z = end - nt;  // inst_start
            rr = rect[g];
        }
        minx = rr.x & 0xFFFF;
        maxx = rr.y & 0xFFFF;
        const uint32_t miny = rr.x >> 16;
        y0 = miny > (uint32_t)ty0 ? miny : (uint32_t)ty0;
    }
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(end - nt));
    const uint64_t vmask = __ballot(valid);
    if (vmask == 0) return;
    const int last_lane = 63 - __builtin_clzll(vmask);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)end, last_lane) - first;
    s_start[w][lane] = valid ? end - nt - first : 0xFFFFFFFFu;
    s_g[w][lane] = g;
    s_w[w][lane] = maxx - minx;
    s_x0[w][lane] = minx;
    s_y0[w][lane] = y0;
    wave_lds_sync();
    emit_wave(s_start[w], s_g[w], s_w[w], s_x0[w], s_y0[w], first, total, grid_x, cap, tkey, tgid);
}

// ---- presort: each depth rank's binning payload, gathered once into rank order ----
// rtiles[r] = tiles[g], rrect[r] = (rect lo, rect hi, g, 0) for g = the sorted gid at rank r.  The
// reads are random (16 B per visible Gaussian, L2 / MALL-resident), the writes coalesced; the
// scan, F3 and the gather then stream the payload instead of each making random reads.
// It also sums each 256-rank block's tiles_touched into bsum[block] (for the ranked F3's scan).
__global__ __launch_bounds__(256) void rank_payload_kernel(const uint32_t* __restrict__ sgid,
                                                           const uint32_t* __restrict__ tiles,
                                                           const uint4* __restrict__ rect, int n,
                                                           uint32_t* __restrict__ rtiles,
                                                           uint4* __restrict__ rrect, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t wsum[kWaves];
    const int r = blockIdx.x * 256 + threadIdx.x;
    uint32_t nt = 0;
    if (r < n) {
        const uint32_t g = sgid[r];
        nt = tiles[g];
        uint4 q = make_uint4(0u, 0u, g, 0u);
        if (nt) {
            const uint4 rr = rect[g];
            q.x = rr.x;
            q.y = rr.y;
        }
        rtiles[r] = nt;
        rrect[r] = q;
    }
    uint32_t s = nt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- row-bucketed binning: F3 + the tile sort + F5 in two counting passes ----
// The stable tile-key sort of the K emitted instances (two LSD passes over 8-byte records, ~340 MB
// of traffic at 1M / 1080p) is replaced by two counting passes that each touch far fewer bytes:
//   A. (Gaussian, tile row) pairs -- ~2.8 per visible Gaussian against ~7.5 instances -- bucketed by
//      row: a per-block row count (rb_rows_count), the radix column scan, and a placement that
//      takes each pair's slot from an LDS counter of its row (rb_rows_place).  A pair is
//      (gid, x0 | x1 << 16): its columns, not expanded.
//   B. per chunk of kRbChunk pairs of one row: the pairs' columns counted (rb_chunks_count), every
//      row's [column][chunk] counts scanned flat with a look-back over rows (rb_tiles_scan, which
//      also writes the tile ranges), and each chunk's instances placed from LDS column counters,
//      staged in LDS and written as coalesced column runs (rb_chunks_place).
// Result: every tile's entries contiguous and the ranges F5 would write -- ~140 MB of
// traffic and no separate F3 / F5 -- but a tile's entries in arbitrary order: the per-tile depth
// sort that follows orders them by the whole (depth, gid) key (the register forms; with
// `unordered` tile_depth_sort_big puts its depth ties in gid order), so the canonical list is the
// radix path's bit for bit.  Used when
// the image has at most kRbMaxRows tile rows and kRbMaxCols tile columns (row / column ids fit one
// byte; tall grids of at most kRbMaxRows tile rows -- views mode's stacked images included -- take
// it too), outside presort mode, below kRbMaxCap instances (gsr_api.cpp expected_layout; recorded
// in gsr_buffers.layout).
constexpr int kRbChunk = kRbChunkPairs;  // pairs per pass-B block (4 per thread)
static_assert(kRbChunk % 256 == 0 && kRbMaxRows == 256 && kRbMaxCols == 256, "one row / column per thread");
// LDS staging (pairs) of a pass-A block (~720 at 1M / 1080p; a block past it writes unstaged):
// 1024 keeps the block at 16 KB, 8 waves per SIMD (2048: 30 KB, 5)
constexpr int kRbStageA = 1024;
constexpr int kRbStage = 4096;  // LDS staging (instances) of a pass-B block (~2800 at 1M / 1080p)

// rows of one block's Gaussians -> histA[r * nbA + b] (F1 writes the same counts itself when it
// ran for these Gaussians: PreOut.rb_hist; this kernel serves the band side, whose splats arrive
// from the exchange)
__global__ __launch_bounds__(256) void rb_rows_count(const uint32_t* __restrict__ tiles, const uint4* __restrict__ rect,
                                                     int n, int ty0, int ty1, uint32_t* __restrict__ histA, int nbA) {
    __shared__ uint32_t cnt[kRbMaxRows];
    const int tid = threadIdx.x, R = ty1 - ty0;
    cnt[tid] = 0u;
    __syncthreads();
    const int g = blockIdx.x * 256 + tid;
    if (g < n) {
        const uint32_t nt = tiles[g];
        if (nt) {
            const uint4 rr = rect[g];
            const int miny = (int)(rr.x >> 16), maxy = (int)(rr.y >> 16);
            const int by0 = miny > ty0 ? miny : ty0, by1 = maxy < ty1 ? maxy : ty1;
            for (int r = by0; r < by1; ++r) atomicAdd(&cnt[r - ty0], 1u);
        }
    }
    __syncthreads();
    if (tid < R) histA[(size_t)tid * nbA + blockIdx.x] = cnt[tid];
}

// Pairs of the block's 256 Gaussians placed row by row: the block counts its pairs per row in
// LDS, takes each row's global base (the column-scanned counts), and every lane walks its own
// rows, taking a slot of its row from an LDS counter -- the order of a row's pairs inside the
// block is arbitrary (the per-tile sort that follows orders each tile by (depth, gid) itself),
// so no per-row ballot sweep is needed.  Staged in LDS by row, written as coalesced row runs.
__global__ __launch_bounds__(256) void rb_rows_place(const uint32_t* __restrict__ tiles, uint4* __restrict__ rect,
                                                     uint32_t* __restrict__ offsets, const uint32_t* __restrict__ bsum,
                                                     int n, int ty0, int ty1,
                                                     const uint32_t* __restrict__ histA,
                                                     const uint32_t* __restrict__ totA, int nbA,
                                                     uint32_t* __restrict__ pgid, uint32_t* __restrict__ pxr,
                                                     long long pcap, const uint32_t* __restrict__ depth_key,
                                                     uint2* __restrict__ ppair) {
    __shared__ uint32_t cnt[kRbMaxRows];  // pairs per row, then the running staging slot
    __shared__ uint32_t gb[kRbMaxRows];   // global position of the block's first pair of row r
    __shared__ uint32_t lb[kRbMaxRows];   // staging position of the block's first pair of row r
    __shared__ uint32_t sg[kRbStageA], sx[kRbStageA], sk[kRbStageA];
    __shared__ uint8_t sr[kRbStageA];
    __shared__ uint32_t wsum[kWaves];
    const int tid = threadIdx.x, R = ty1 - ty0;
    cnt[tid] = 0u;
    // the row totals and this block's column of the scanned counts: loads issued first (they do
    // not depend on the Gaussians), waited for at the block scan
    const uint32_t ta = tid < R ? totA[tid] : 0u;
    const uint32_t ha = tid < R ? histA[(size_t)tid * nbA + blockIdx.x] : 0u;
    const int g = blockIdx.x * 256 + tid;
    int by0 = 0, by1 = 0;  // band-relative rows
    uint32_t xr = 0;
    const uint32_t nt = g < n ? tiles[g] : 0u;
    uint32_t incl;  // F2: the inclusive scan of tiles_touched at g
    if (bsum) {     // from F1's scanned block sums: this block's base + the in-block scan
        const uint32_t bb = bsum[blockIdx.x];
        uint32_t tdum;
        incl = bb + block_exclusive_scan(nt, wsum, &tdum) + nt;
        if (g < n) offsets[g] = incl;
    } else {
        incl = g < n ? offsets[g] : 0u;  // the three-kernel scan's
    }
    if (nt) {
        const uint4 rr = rect[g];
        rect[g].z = incl - nt;  // inst_start: the emission index of the first instance (F3's)
        const int miny = (int)(rr.x >> 16), maxy = (int)(rr.y >> 16);
        by0 = (miny > ty0 ? miny : ty0) - ty0;
        by1 = (maxy < ty1 ? maxy : ty1) - ty0;
        xr = (rr.x & 0xFFFFu) | (rr.y << 16);
    }
    const uint32_t dk = ppair && nt ? depth_key[g] : 0u;  // the pair's depth key (ppair: for pass B)
    __syncthreads();
    for (int r = by0; r < by1; ++r) atomicAdd(&cnt[r], 1u);
    __syncthreads();
    uint32_t tot;
    {
        const uint32_t c = cnt[tid];
        uint32_t sdum;
        const uint32_t rowbase = block_exclusive_scan(ta, wsum, &sdum);
        gb[tid] = tid < R ? rowbase + ha : 0u;
        lb[tid] = block_exclusive_scan(c, wsum, &tot);
        cnt[tid] = 0u;
    }
    __syncthreads();
    const bool staged = tot <= (uint32_t)kRbStageA;  // block-uniform
    for (int r = by0; r < by1; ++r) {
        const uint32_t k = atomicAdd(&cnt[r], 1u);
        if (staged) {
            sg[lb[r] + k] = (uint32_t)g;
            sx[lb[r] + k] = xr;
            if (ppair) sk[lb[r] + k] = dk;
            sr[lb[r] + k] = (uint8_t)r;
        } else {
            const long long pos = (long long)gb[r] + k;
            if (pos < pcap) {
                if (ppair) ppair[pos] = make_uint2((uint32_t)g, dk);
                else pgid[pos] = (uint32_t)g;
                pxr[pos] = xr;
            }
        }
    }
    if (!staged) return;
    __syncthreads();
    for (int i = tid; i < (int)tot; i += 256) {
        const int rr = sr[i];
        const long long pos = (long long)gb[rr] + (uint32_t)i - lb[rr];
        if (pos < pcap) {
            if (ppair) ppair[pos] = make_uint2(sg[i], sk[i]);
            else pgid[pos] = sg[i];
            pxr[pos] = sx[i];
        }
    }
}

// Pass-B chunk numbering (every pass-B kernel the same): row r holds ceil(pairs_r / kRbChunk)
// chunks of its pairs (pairs clamped to the pair capacity), numbered in row order.  Each block
// builds the rows' pair and chunk bases once in LDS (two block scans over the rows) and then finds
// a chunk's row by a binary search there.
struct RbRows {
    uint32_t pbase[kRbMaxRows];  // the row's first pair
    uint32_t cbase[kRbMaxRows];  // the row's first chunk
    uint32_t npair[kRbMaxRows];  // the row's pairs (clamped)
    uint32_t wsum[kWaves];
    uint32_t nchunks;            // all rows' chunks
};

__device__ __forceinline__ void rb_rows_table(const uint32_t* __restrict__ totA, int R, long long pcap, RbRows& t) {
    const int tid = threadIdx.x;
    const uint32_t ta = tid < R ? totA[tid] : 0u;
    uint32_t tp;
    const uint32_t pb = block_exclusive_scan(ta, t.wsum, &tp);
    const long long avail = pcap - (long long)pb;
    const uint32_t tc = avail <= 0 ? 0u : (avail < (long long)ta ? (uint32_t)avail : ta);
    uint32_t tcs;
    const uint32_t cb = block_exclusive_scan((tc + kRbChunk - 1) / kRbChunk, t.wsum, &tcs);
    t.pbase[tid] = pb;
    t.cbase[tid] = tid < R ? cb : 0xFFFFFFFFu;  // rows past R never match
    t.npair[tid] = tc;
    if (tid == 0) t.nchunks = tcs;
    __syncthreads();
}

struct RbChunk {
    int r, k, nch;
    uint32_t p0, p1, cp;  // pairs [p0, p1); cp: the row's first chunk
};

__device__ __forceinline__ RbChunk rb_chunk(const RbRows& t, uint32_t b) {
    // the last row whose first chunk is <= b: a row without chunks shares its first chunk number with
    // the next row that has some, so the last such row is the one holding chunk b
    int r = 0;
#pragma unroll
    for (int step = kRbMaxRows / 2; step > 0; step >>= 1)
        if (t.cbase[r + step] <= b) r += step;
    RbChunk ch;
    ch.r = r;
    ch.cp = t.cbase[r];
    ch.k = (int)(b - ch.cp);
    ch.nch = (int)((t.npair[r] + kRbChunk - 1) / kRbChunk);
    ch.p0 = t.pbase[r] + (uint32_t)ch.k * kRbChunk;
    const uint32_t end = t.pbase[r] + t.npair[r];
    ch.p1 = ch.p0 + kRbChunk < end ? ch.p0 + kRbChunk : end;
    return ch;
}

// pass B, counts: instances of each chunk per column -> histB[gx * cp + c * nch + k].  Blocks walk
// the chunks (grid-stride), so a grid sized for the worst case costs no empty blocks.
__global__ __launch_bounds__(256) void rb_chunks_count(const uint32_t* __restrict__ pxr, const uint32_t* __restrict__ totA,
                                                       int R, int gx, long long pcap, uint32_t* __restrict__ histB) {
    __shared__ RbRows t;
    __shared__ uint32_t cnt[kRbMaxCols];
    const int tid = threadIdx.x;
    rb_rows_table(totA, R, pcap, t);
    for (uint32_t b = blockIdx.x; b < t.nchunks; b += gridDim.x) {
        const RbChunk ch = rb_chunk(t, b);
        cnt[tid] = 0u;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kRbChunk / 256; ++q) {
            const uint32_t p = ch.p0 + q * 256 + tid;
            if (p < ch.p1) {
                const uint32_t xr = pxr[p];
                for (uint32_t c = xr & 0xFFFFu; c < (xr >> 16); ++c) atomicAdd(&cnt[c], 1u);
            }
        }
        __syncthreads();
        if (tid < gx) histB[(size_t)gx * ch.cp + (size_t)tid * ch.nch + ch.k] = cnt[tid];
    }
}

// pass B, scan: the [column][chunk] counts of every row, flat, in R x G partitions -- partition
// p = r G + g holds columns [g gx / G, (g + 1) gx / G) of row r, contiguous in the flat order.
// Each block scans one partition (exclusive), takes its global base by a decoupled look-back over
// the partitions before it (in dispatch order: a ticket), and stores global positions in place;
// then the tile ranges of its columns ((0, 0) for an empty tile, as F5 leaves it; clamped to
// cap).  G > 1 spreads a row over several CUs: a band of 8 tile rows was 8 blocks on the chip
// (~22 us at 5M, the same as 68 rows of the full image).
constexpr int kRbScanThreads = 1024, kRbScanQ = 32;
// The look-back's status words pack a 30-bit count: the layout word keeps this binning to
// capacities below 2^30 (gsr_api.cpp expected_layout), so a step within its capacity never
// counts past it.  A look-back that spins past its bound (never expected) publishes what it has
// and marks the step: K_dev = UINT32_MAX, which every reader of K takes for an overflow
// (gsr_read_num_rendered names the cause), so the ranges it leaves are never trusted silently.
__global__ __launch_bounds__(kRbScanThreads) void rb_tiles_scan(const uint32_t* __restrict__ totA, int R, int gx,
                                                                int ty0, long long pcap, long long cap,
                                                                uint32_t* __restrict__ histB,
                                                                uint32_t* __restrict__ status,
                                                                uint32_t* __restrict__ ticket,
                                                                uint2* __restrict__ ranges,
                                                                uint32_t* __restrict__ K_dev, int G) {
    __shared__ uint32_t wsum[kRbScanThreads / 64];
    __shared__ uint32_t tstart[kRbMaxCols];
    __shared__ uint32_t s_row[2];
    __shared__ int s_p;
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_p = (int)atomicAdd(ticket, 1u);  // partitions in dispatch order (the look-back's progress)
    __syncthreads();
    const int p = s_p, r = p / G, gi = p - r * G;
    const int c0 = gi * gx / G, c1 = (gi + 1) * gx / G;  // this partition's columns
    // the row's chunks, as rb_rows_table numbers them
    {
        const uint32_t ta = tid < R ? totA[tid] : 0u;
        uint32_t tp;
        const uint32_t pb = block_exclusive_scan(ta, wsum, &tp);
        const long long avail = pcap - (long long)pb;
        const uint32_t tc = avail <= 0 ? 0u : (avail < (long long)ta ? (uint32_t)avail : ta);
        const uint32_t nc = (tc + kRbChunk - 1) / kRbChunk;
        uint32_t tcs;
        const uint32_t cb = block_exclusive_scan(nc, wsum, &tcs);
        if (tid == r) {
            s_row[0] = nc;
            s_row[1] = cb;
        }
        __syncthreads();
    }
    const uint32_t nch = s_row[0], cp = s_row[1];
    uint32_t* const h = histB + (size_t)gx * cp + (size_t)c0 * nch;  // the partition's counts
    const uint32_t E = (uint32_t)(c1 - c0) * nch;
    // the common case: the partition's counts in registers, Q consecutive ones per thread (up to
    // kRbScanQ x 1024), one block scan and one write of the final positions
    const uint32_t Q = (E + kRbScanThreads - 1) / kRbScanThreads;
    const bool one = Q <= (uint32_t)kRbScanQ;
    const uint32_t i0 = Q * tid;
    uint32_t cnts[kRbScanQ], excl = 0, carry = 0;
    if (one) {
        uint32_t sv = 0;
#pragma unroll
        for (int q = 0; q < kRbScanQ; ++q) {
            cnts[q] = (uint32_t)q < Q && i0 + q < E ? h[i0 + q] : 0u;
            sv += cnts[q];
        }
        excl = block_exclusive_scan(sv, wsum, &carry);
    } else {
        for (uint32_t base = 0; base < E; base += 4 * kRbScanThreads) {
            const uint32_t j0 = base + 4 * tid;  // (partitions past kRbScanQ x 1024 counts: rounds of 4 per thread)
            uint32_t v[4], sv = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = j0 + q < E ? h[j0 + q] : 0u;
                sv += v[q];
            }
            uint32_t tot;
            uint32_t run = carry + block_exclusive_scan(sv, wsum, &tot);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (j0 + q < E) h[j0 + q] = run;  // partition-relative for now
                run += v[q];
            }
            carry += tot;
        }
    }
    // look-back (wave 0): the instances of the partitions before p
    if (tid < 64) {
        uint32_t excl = 0;
        if (p == 0) {
            if (lane == 0) __hip_atomic_store(status, kInc | carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(status + p, kAgg | carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int pos = p - 1;
            uint32_t spins = 0;
            while (true) {
                const int idx = pos - lane;
                uint32_t v = kInc;
                if (idx >= 0) v = __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (__ballot((v & ~kCntMask) == 0u)) {
                    if (++spins > (1u << 24)) break;  // never expected; bounded so a bug cannot hang
                    __builtin_amdgcn_s_sleep(1);
                    if (idx >= 0 && (v & ~kCntMask) == 0u)
                        v = __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const uint64_t inc = __ballot((v & kInc) != 0u);
                const int k = inc ? __builtin_ctzll(inc) : 64;
                uint32_t c = lane <= k ? (v & kCntMask) : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
                excl += c;
                if (inc || spins > (1u << 24)) break;
                pos -= 64;
            }
            if (lane == 0) __hip_atomic_store(status + p, kInc | (excl + carry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (spins > (1u << 24) && lane == 0 && K_dev) *K_dev = 0xFFFFFFFFu;  // the step is void
        }
        if (lane == 0) s_base = excl;
    }
    __syncthreads();
    const uint32_t pbase = s_base;  // the global position of the partition's first instance
    if (one) {
        uint32_t run = pbase + excl;
        uint32_t c = i0 / (nch ? nch : 1u), k = i0 - c * nch;  // column (partition-relative) and chunk of i0
#pragma unroll
        for (int q = 0; q < kRbScanQ; ++q) {
            if ((uint32_t)q < Q && i0 + q < E) {
                h[i0 + q] = run;
                if (k == 0) tstart[c0 + c] = run;
                run += cnts[q];
                if (++k == nch) k = 0, ++c;
            }
        }
    } else {
        for (uint32_t i = tid; i < E; i += kRbScanThreads) h[i] += pbase;
        __syncthreads();
        if (tid >= c0 && tid < c1 && nch) tstart[tid] = h[(size_t)(tid - c0) * nch];
    }
    __syncthreads();
    // tile c of the partition: [its first chunk's base, the next tile's); the partition's last
    // tile ends where the next partition starts (flat order)
    if (tid >= c0 && tid < c1) {
        const uint32_t a = nch ? tstart[tid] : pbase, e = tid + 1 < c1 && nch ? tstart[tid + 1] : pbase + carry;
        const long long a2 = a < cap ? a : cap, e2 = e < cap ? e : cap;
        ranges[(size_t)(ty0 + r) * gx + tid] = e2 > a2 ? make_uint2((uint32_t)a2, (uint32_t)e2) : make_uint2(0u, 0u);
    }
}

// pass B, placement: each chunk's instances, a slot per instance from its column's LDS counter
// (order inside a tile is free, as in pass A), staged in LDS by column and written as coalesced
// column runs (the gid; with tpair the (gid, depth key) pair, the key from pass A's
// ppair, so the per-tile sort that follows reads its keys coalesced instead of gathering one
// behind every gid load, one 8-B store per instance).  The staging holds each instance's pair
// index (16 bits) and column; the chunk's pairs (gid, key) sit in LDS beside it.
constexpr int kRbPlaceWpe = 1;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kRbPlaceWpe))) void rb_chunks_place(const uint32_t* __restrict__ pgid, const uint32_t* __restrict__ pxr,
                                                       const uint32_t* __restrict__ totA, int R, int gx,
                                                       long long pcap, long long cap,
                                                       const uint32_t* __restrict__ histB,
                                                       uint32_t* __restrict__ tgid,
                                                       const uint2* __restrict__ ppair,
                                                       uint2* __restrict__ tpair) {
    __shared__ RbRows t;
    __shared__ uint32_t cnt[kRbMaxCols];  // instances per column, then the running staging slot
    __shared__ uint32_t lb[kRbMaxCols];   // staging start of column c
    __shared__ uint32_t gb[kRbMaxCols];   // global position of the chunk's first instance of column c
    __shared__ uint32_t pg[kRbChunk], pk[kRbChunk];  // the chunk's pairs: gid, depth key
    // staged instance: pair index | column << 16, one word per instance (no sub-dword LDS stores
    // from neighbouring lanes into one dword)
    __shared__ uint32_t spc[kRbStage];
    __shared__ uint32_t wsum[kWaves];
    static_assert(kRbChunk <= 65536, "u16 pair index");
    const int tid = threadIdx.x;
    const bool keys = tpair != nullptr;  // launch-uniform
    rb_rows_table(totA, R, pcap, t);
    constexpr int kQ = kRbChunk / 256;
    // the next chunk's pairs are loaded while this one is placed (register double buffer)
    uint32_t nxr[kQ], ngg[kQ], nkk[kQ];
    auto load_pairs = [&](uint32_t b) {
        const RbChunk c = rb_chunk(t, b);
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const uint32_t p = c.p0 + q * 256 + tid;
            nxr[q] = p < c.p1 ? pxr[p] : 0u;  // 0: no columns
            if (keys) {
                const uint2 pp = p < c.p1 ? ppair[p] : make_uint2(0u, 0u);
                ngg[q] = pp.x;
                nkk[q] = pp.y;
            } else {
                ngg[q] = p < c.p1 ? pgid[p] : 0u;
                nkk[q] = 0u;
            }
        }
    };
    if (blockIdx.x < t.nchunks) load_pairs(blockIdx.x);
    for (uint32_t b = blockIdx.x; b < t.nchunks; b += gridDim.x) {
        const RbChunk ch = rb_chunk(t, b);
        cnt[tid] = 0u;
        const uint32_t hb = tid < gx ? histB[(size_t)gx * ch.cp + (size_t)tid * ch.nch + ch.k] : 0u;
        uint32_t xr[kQ], gg[kQ], kk[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            xr[q] = nxr[q];
            gg[q] = ngg[q];
            kk[q] = nkk[q];
        }
        if (b + gridDim.x < t.nchunks) load_pairs(b + gridDim.x);
        __syncthreads();  // cnt zeroed (and the previous chunk's staging read out)
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            for (uint32_t c = xr[q] & 0xFFFFu; c < (xr[q] >> 16); ++c) atomicAdd(&cnt[c], 1u);
        __syncthreads();
        uint32_t tot;
        {
            const uint32_t c = cnt[tid];
            lb[tid] = block_exclusive_scan(c, wsum, &tot);
            gb[tid] = hb;
            cnt[tid] = 0u;
        }
        __syncthreads();
        const bool staged = tot <= (uint32_t)kRbStage;  // block-uniform
        if (staged) {
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                pg[q * 256 + tid] = gg[q];
                if (keys) pk[q * 256 + tid] = kk[q];
            }
        }
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            for (uint32_t c = xr[q] & 0xFFFFu; c < (xr[q] >> 16); ++c) {
                const uint32_t k = atomicAdd(&cnt[c], 1u);
                if (staged) {
                    spc[lb[c] + k] = (uint32_t)(q * 256 + tid) | (c << 16);
                } else {
                    const long long pos = (long long)gb[c] + k;
                    if (pos < cap) {
                        if (keys) tpair[pos] = make_uint2(gg[q], kk[q]);
                        else tgid[pos] = gg[q];
                    }
                }
            }
        }
        if (staged) {
            __syncthreads();
            for (int i = tid; i < (int)tot; i += 256) {
                const uint32_t pc = spc[i];
                const int c = (int)(pc >> 16);
                const long long pos = (long long)gb[c] + ((uint32_t)i - lb[c]);
                if (pos < cap) {
                    const int pi = (int)(pc & 0xFFFFu);
                    if (keys) tpair[pos] = make_uint2(pg[pi], pk[pi]);
                    else tgid[pos] = pg[pi];
                }
            }
        }
        __syncthreads();  // cnt / lb / gb / staging reused by the next chunk
    }
}

// ---- F5 finalize: tile ranges from the sorted keys ----
// Four sorted keys per thread (one 16-B load; the sorted array is 16-B aligned), the neighbours
// across the quad from the adjacent words (cache hits): 0.075 -> ~0.03 ms at 5M / 1080p.
constexpr int kFinQ = 4;
__global__ __launch_bounds__(256) void finalize_kernel(const uint32_t* __restrict__ stile, long long cap,
                                                       const uint32_t* __restrict__ n_dev,
                                                       uint2* __restrict__ ranges) {
    const long long K = live_count(cap, n_dev);
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * kFinQ;
    if (i0 >= K) return;
    uint32_t t[kFinQ];
    if (i0 + kFinQ <= K) {
        const uint4 q = *reinterpret_cast<const uint4*>(stile + i0);
        t[0] = q.x, t[1] = q.y, t[2] = q.z, t[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kFinQ; ++j) t[j] = i0 + j < K ? stile[i0 + j] : 0xFFFFFFFFu;
    }
    uint32_t prev = i0 > 0 ? stile[i0 - 1] : 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < kFinQ; ++j) {
        const long long i = i0 + j;
        if (i >= K) break;
        const uint32_t next = j + 1 < kFinQ ? t[j + 1] : (i + 1 < K ? stile[i + 1] : 0xFFFFFFFFu);
        if (i == 0 || prev != t[j]) ranges[t[j]].x = (uint32_t)i;
        if (i == K - 1 || next != t[j]) ranges[t[j]].y = (uint32_t)(i + 1);
        prev = t[j];
    }
}

}  // namespace

int launch_scan(const uint32_t* tiles, int n, uint32_t* offsets, uint32_t* scan_partials_buf, uint32_t* total_out,
                hipStream_t s, bool fused_ok) {
    if (n <= 0) return (int)hipMemsetAsync(total_out, 0, sizeof(uint32_t), s);
    if (fused_ok && n <= kFusedScanMax) return 0;  // scanned by the fused kernel in launch_duplicate
    const int nb = sort_blocks(n);
    hipLaunchKernelGGL(scan_reduce, dim3(nb), dim3(kB), 0, s, tiles, n, scan_partials_buf);
    hipLaunchKernelGGL(scan_partials, dim3(1), dim3(1024), scan_lds_bytes(nb), s, scan_partials_buf, nb, total_out);
    hipLaunchKernelGGL(scan_downsweep, dim3(nb), dim3(kB), 0, s, tiles, n, scan_partials_buf, offsets);
    return (int)hipGetLastError();
}

// one block of 256 Gaussians: offsets = its scanned base + the in-block inclusive scan
__global__ __launch_bounds__(256) void block_offsets_kernel(const uint32_t* __restrict__ tiles, int n,
                                                            const uint32_t* __restrict__ bsum,
                                                            uint32_t* __restrict__ offsets) {
    __shared__ uint32_t wsum[kWaves];
    const int g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t nt = g < n ? tiles[g] : 0u;
    uint32_t tdum;
    const uint32_t incl = bsum[blockIdx.x] + block_exclusive_scan(nt, wsum, &tdum) + nt;
    if (g < n) offsets[g] = incl;
}

int launch_scan_blocks(uint32_t* bsum, int n, uint32_t* total_out, hipStream_t s) {
    if (n <= 0) return (int)hipMemsetAsync(total_out, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(scan_partials, dim3(1), dim3(1024), scan_lds_bytes(div_up(n, 256)), s, bsum, div_up(n, 256),
                       total_out);
    return (int)hipGetLastError();
}

int launch_block_offsets(const uint32_t* tiles, int n, const uint32_t* bsum, uint32_t* offsets, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(block_offsets_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, tiles, n, bsum, offsets);
    return (int)hipGetLastError();
}

int launch_rb_binning(const uint32_t* tiles, uint4* rect, uint32_t* offsets, int n, int gx, int ty0, int ty1,
                      uint32_t* histA, uint32_t* histB, uint32_t* rb_status, uint32_t* pgid, uint32_t* pxr,
                      uint32_t* tgid, uint2* ranges, long long cap, hipStream_t s,
                      bool rows_counted, const uint32_t* bsum, uint32_t* K_dev, const uint32_t* depth_key,
                      uint2* ppair, uint2* tpair) {
    const int R = ty1 - ty0;
    if (!depth_key || !ppair || !tpair) ppair = tpair = nullptr;
    if (n <= 0 || R <= 0 || cap <= 0) return 0;  // ranges stay cleared
    if (R > kRbMaxRows || gx > kRbMaxCols || cap >= kRbMaxCap) return (int)hipErrorInvalidValue;
    const int nbA = div_up(n, 256);
    uint32_t* const totA = histA + (size_t)256 * nbA;
    if (!rows_counted)
        hipLaunchKernelGGL(rb_rows_count, dim3(nbA), dim3(256), 0, s, tiles, rect, n, ty0, ty1, histA, nbA);
    hipLaunchKernelGGL(rb_colscan, dim3(R), dim3(1024), scan_lds_bytes(nbA), s, histA, nbA, totA);
    hipLaunchKernelGGL(rb_rows_place, dim3(nbA), dim3(256), 0, s, tiles, rect, offsets, bsum, n, ty0, ty1, histA, totA,
                       nbA, pgid, pxr, cap, depth_key, ppair);
    // chunks: at most cap / kRbChunk full ones plus one partial per row; the blocks walk them, so
    // the grid is capped near what the chip holds at once (no tail of empty blocks)
    const int nch_max = div_up(cap, kRbChunk) + R;
    const int gcount = nch_max < 2048 ? nch_max : 2048, gplace = nch_max < 1280 ? nch_max : 1280;
    hipLaunchKernelGGL(rb_chunks_count, dim3(gcount), dim3(256), 0, s, pxr, totA, R, gx, cap, histB);
    // partitions per row: enough to spread a band's few rows over the chip, at most kRbScanSplit
    int G = kRbScanSplit < 256 / R ? kRbScanSplit : 256 / R;
    G = G < 1 ? 1 : G > gx ? gx : G;
    hipLaunchKernelGGL(rb_tiles_scan, dim3(R * G), dim3(kRbScanThreads), 0, s, totA, R, gx, ty0, cap, cap, histB,
                       rb_status + 16, rb_status, ranges, K_dev, G);
    hipLaunchKernelGGL(rb_chunks_place, dim3(gplace), dim3(256), 0, s, pgid, pxr, totA, R, gx, cap, cap, histB,
                       tgid, ppair, tpair);
    return (int)hipGetLastError();
}

int launch_duplicate(const uint32_t* tiles, uint4* rect, int n, int grid_x, int ty0, uint32_t* offsets,
                     uint32_t* lookback, uint32_t* tkey, uint32_t* tgid, long long cap, uint32_t* total_out,
                     hipStream_t s, bool scanned) {
    if (n <= 0) return 0;
    if (n <= kFusedScanMax && !scanned) {  // fused look-back scan + duplicate
        const int nb = div_up(n, 256);
        if (hipError_t e = hipMemsetAsync(lookback, 0, sizeof(uint32_t) * (16 + (size_t)nb), s)) return (int)e;
        hipLaunchKernelGGL(scan_duplicate_kernel, dim3(nb), dim3(256), 0, s, tiles, rect, n, grid_x, ty0, offsets,
                           tkey, tgid, cap, lookback + 16, lookback, total_out);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(duplicate_kernel<false>, dim3(div_up(n, 256)), dim3(256), 0, s, offsets, tiles, rect,
                       nullptr, n, grid_x, ty0, tkey, tgid, cap, nullptr);
    return (int)hipGetLastError();
}

int launch_depth_presort(const uint32_t* depth_key, const uint32_t* tiles, const uint4* rect, int n, uint32_t* dk0,
                         uint32_t* dv0, uint32_t* dk1, uint32_t* dv1, uint32_t* hist, uint32_t* rtiles, uint4* rrect,
                         uint32_t* bsum, uint32_t* total_out, hipStream_t s) {
    if (n <= 0) return (int)hipMemsetAsync(total_out, 0, sizeof(uint32_t), s);
    int which = -1;  // 4 passes of 8 bits: the result lands in (dk1, dv1)
    if (int e = radix_sort(depth_key, nullptr, dk0, dv0, dk1, dv1, n, nullptr, 32, hist, &which, s)) return e;
    const uint32_t* sgid = which == 0 ? dv0 : dv1;
    const int nb = div_up(n, 256);
    hipLaunchKernelGGL(rank_payload_kernel, dim3(nb), dim3(256), 0, s, sgid, tiles, rect, n, rtiles, rrect, bsum);
    // the 256-rank blocks' exclusive offsets and K: F3 (launch_duplicate_ranked) scans inside them
    hipLaunchKernelGGL(scan_partials, dim3(1), dim3(1024), scan_lds_bytes(nb), s, bsum, nb, total_out);
    return (int)hipGetLastError();
}

int launch_duplicate_ranked(const uint32_t* rtiles, const uint4* rrect, uint4* rect, int n, int grid_x, int ty0,
                            const uint32_t* bexcl, uint32_t* offsets, uint32_t* tkey, uint32_t* tgid, long long cap,
                            hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(duplicate_kernel<true>, dim3(div_up(n, 256)), dim3(256), 0, s, offsets, rtiles, rect, rrect, n,
                       grid_x, ty0, tkey, tgid, cap, bexcl);
    return (int)hipGetLastError();
}

// the GSR_VIEW_SORTED_TILE accessor's tile keys (gsr_kernels.h)
__global__ __launch_bounds__(256) void tile_keys_from_ranges(const uint2* __restrict__ ranges, long long cap,
                                                             uint32_t* __restrict__ tkey) {
    const uint2 rg = ranges[blockIdx.x];
    const uint32_t e = rg.y < cap ? rg.y : (uint32_t)cap;
    for (uint32_t i = rg.x + threadIdx.x; i < e; i += 256) tkey[i] = blockIdx.x;
}

int launch_tile_keys_from_ranges(const uint2* ranges, int tiles, long long cap, uint32_t* tkey, hipStream_t s) {
    if (tiles <= 0 || cap <= 0) return 0;
    hipLaunchKernelGGL(tile_keys_from_ranges, dim3(tiles), dim3(256), 0, s, ranges, cap, tkey);
    return (int)hipGetLastError();
}

int launch_finalize(const uint32_t* sorted_tile, long long cap, const uint32_t* K_dev, uint2* ranges, hipStream_t s) {
    if (cap <= 0) return 0;
    hipLaunchKernelGGL(finalize_kernel, dim3(div_up(div_up(cap, kFinQ), 256)), dim3(256), 0, s, sorted_tile, cap, K_dev,
                       ranges);
    return (int)hipGetLastError();
}

}  // namespace gsr
