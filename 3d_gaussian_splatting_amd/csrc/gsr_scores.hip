// gsr_scores.hip -- per-Gaussian importance scores of one rendered view (gsr_forward_scores) on
// gfx950: a replay of F6 that keeps, per (tile, record), three moments of the blending weight
// w = T alpha over the tile's pixels -- max w, sum w, the number of contributing pixels -- and a
// per-Gaussian gather of them in emission order.
//
// Replay.  One wave per (tile, chunk), all four 16x4 stripes, F6's pixel layout (lane l: column
// l & 15, row l >> 4 of each stripe).  alpha and T are recomputed with F6's own text
// (gsr_blend_dev.h: pair_alpha_keep, the Horner exponent, T - alpha T, the >= 1e-4 test, the sign
// of T as the finished flag) under F6's compile flags, so the contributing (pixel, Gaussian) pairs
// and the termination point are the forward's -- the same set B1 differentiates.  What the forward
// left behind is used the way B1 uses it: the per-entry stripe masks `mk` pick the entries that can
// touch a live stripe before any record is loaded (up to 64 of the next 256), the `term` table ends
// the walk at the tile's termination index and names the chunk starts, and chunk c > 0 resumes
// from F6's checkpoint (T in ck.x, a stripe F6 did not write starts dead).  Chunks keep the tail of
// a deep tile short exactly as they do for B1; the colour sums of the checkpoint are not read.
//
// Per visited record the wave counts the contributing pixels on the scalar port (the popcount of
// the stripes' contributor masks), reduces max w and sum w over each quad by DPP, and parks the 16
// quad partials in LDS; every kScPark records one (record, moment) output per lane is finished
// from LDS in fixed quad order and stored at the record's emission index j -- the index B1 derives
// from rect[g].z and the tile's place in the rect; j >= cap is dropped as B1 drops it.  Plain
// stores, one writer per entry, no atomics: two calls give the same bits.  Records without a
// contributing pixel write nothing; the entry's flag byte (cleared by the launcher, cap bytes)
// tells the gather which entries exist.
//
// No colour, no R chain, no dL/dpix: 9 live VGPRs of pixel state (T and the row of four stripes,
// the column), so the kernel runs at the 8 waves per SIMD the hardware allows -- 4,352 B of LDS per
// one-wave block (2,048 staged records + 2,176 parking + 128 of j / count words) is 37 blocks per
// 160-KiB CU, above the 32 that 8 waves per SIMD need.
#include "gsr_blend_dev.h"

namespace gsr {
namespace {

template <int CTRL>
__device__ inline float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

// Parking: kScPark records of 16 quads x (max, sum).  The flush lane of (slot s, moment c) reads
// words s kScSlot + c + 2 i, i < 16; with kScSlot = 34 its bank is (2 s + c + 2 i) mod 32, and the
// 32 flush lanes (s < 16, c < 2: one ds_read_b32 lane group) sit on 32 different banks at every i.
constexpr int kScPark = 16;
constexpr int kScSlot = 34;
static_assert(2 * kScPark <= 32 && kScSlot % 2 == 0, "one lane group flushes; float2 stores of the quad leaders");

struct ScoreOut {
    float* mx;      // per entry: max over the tile's pixels of w
    float* sm;      //            sum
    uint32_t* ct;   //            contributing pixels
    uint8_t* fl;    //            1 where the replay wrote the entry
};

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void score_replay_kernel(
    const BlendGeom geo, const uint2* __restrict__ ranges, const uint32_t* __restrict__ sorted_gid,
    const uint4* __restrict__ rect, const float4* __restrict__ rec, const ScoreOut out,
    const uint32_t* __restrict__ term, const float4* __restrict__ ck, const uint8_t* __restrict__ mk) {
    constexpr int SPW = kPPL;  // the wave's stripes: all of the tile's
    __shared__ struct {
        float4 srec[64 * 2];  // per batch slot: (x, y, a', b'), (c', log2 o, emission index, -)
        // the batch selection's tables share the parking bytes, as in B1: they are read back before
        // the batch's first record is parked and rewritten after its last flush (one wave)
        union {
            float qpark[kScPark * kScSlot];
            struct {
                uint32_t sidx[64];  // the batch's entries (list offsets), in list order
                uint32_t smv[64];   // their stripe masks
                uint32_t sgd[64];   // their gids
            };
        };
        uint2 sjc[kScPark];  // per parked record: emission index, contributing pixels
    } lds;
    const int lane = threadIdx.x;
    int tl, chunk;
    {  // block -> (tile, chunk): B1's map (each XCD a contiguous tile range, chunk-major)
        const int q = geo.nwg / 8, r = geo.nwg % 8, xcd = blockIdx.x % 8, local = (int)(blockIdx.x / 8);
        const int t0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, nt = q + (xcd < r ? 1 : 0);
        const int per = q + 1;
        chunk = local / per;
        const int i = local - chunk * per;
        if (i >= nt) return;
        tl = t0 + i;
    }
    const int tile = tl + geo.ty0 * geo.grid_x;
    const uint2 range = ranges[tile];
    const int n_all = (int)(range.y - range.x);
    const uint32_t* table = term + (size_t)tl * kMaxChunks;
    const uint32_t tend = table[0];
    const uint32_t start_u = chunk == 0 ? 0u : table[chunk];
    if (start_u >= (uint32_t)n_all || start_u >= tend) return;  // no such chunk, or all finished before it
    const int start = (int)start_u;
    const uint32_t next = chunk + 1 < kMaxChunks ? table[chunk + 1] : 0xFFFFFFFFu;
    const int n = next < (uint32_t)n_all ? (int)next : n_all;
    const int tx = tile % geo.grid_x, ty = tile / geo.grid_x;
    const int px = tx * kTile + (lane & 15);
    const float pfx = (float)px;
    const int view = ty / geo.vgy, tyl = ty - view * geo.vgy;
    float pfy[SPW], T[SPW];
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        const int pyl = tyl * kTile + (lane >> 4) + 4 * p;
        pfy[p] = (float)pyl;
        T[p] = (px < geo.W && pyl < geo.vh) ? 1.0f : -1.0f;  // a pixel outside the image never counts
    }
    if (chunk > 0) {  // resume from F6's checkpoint: its lane of stripe p is this lane
        const size_t slot = ck_slot_of(geo.ck_fixed, range.x, tl, chunk);
        const float4* src = ck + slot * 256;
        const uint32_t on = *reinterpret_cast<const uint32_t*>(
            reinterpret_cast<const uint8_t*>(ck + (size_t)geo.ck_slots * 256) + 4 * slot);
#pragma unroll
        for (int p = 0; p < SPW; ++p) T[p] = ((on >> (8 * p)) & 0xFFu) ? src[64 * p + lane].x : -1.0f;
    }
    const int n_lim = n < (int)tend ? n : (int)tend;
    const int fs = lane >> 1, fc = lane & 1;  // flush lane: slot, moment
    auto flush = [&](int parked) {
        __syncthreads();  // one-wave block: orders the quad leaders' LDS writes before the reads
        if (fs < parked) {
            const float* q = lds.qpark + fs * kScSlot + fc;
            float t[4] = {-0.f, -0.f, -0.f, -0.f};
            float m = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = q[2 * i];
                t[i & 3] += v;
                m = fmaxf(m, v);
            }
            const uint2 jc = lds.sjc[fs];
            if (jc.x != 0xFFFFFFFFu) {  // an entry past the capacity (binning overflow) has none
                if (fc == 0) {
                    out.mx[jc.x] = m;
                    out.ct[jc.x] = jc.y;
                    out.fl[jc.x] = 1;
                } else {
                    out.sm[jc.x] = (t[0] + t[1]) + (t[2] + t[3]);
                }
            }
        }
        __syncthreads();
    };
    for (int base = start; base < n_lim;) {
        uint32_t live = 0;
#pragma unroll
        for (int p = 0; p < SPW; ++p) live |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
        if (live == 0) break;
        // the batch: up to 64 entries with a live stripe among the next 256, in list order (B1's
        // selection: one aligned mask word and the window's four gids per lane)
        static_assert(kB1Win == 4, "one mask word and four gids per lane");
        const uint32_t a0 = (range.x + (uint32_t)base) & ~(uint32_t)(kB1Win - 1);
        const uint32_t wd = *reinterpret_cast<const uint32_t*>(mk + a0 + 4 * lane);
        const uint4 gw = *reinterpret_cast<const uint4*>(sorted_gid + a0 + 4 * lane);
        const uint32_t gwa[4] = {gw.x, gw.y, gw.z, gw.w};
        uint32_t vis = 0;
#pragma unroll
        for (int i = 0; i < kB1Win; ++i) {
            const int e = (int)(a0 + kB1Win * lane + i - range.x);
            const uint32_t m = (wd >> (8 * i)) & 0xFu;
            if (e >= base && e < n_lim && (m & live)) vis |= 1u << i;
        }
        const uint32_t c = (uint32_t)__popc(vis);
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        const uint32_t total = (uint32_t)__shfl(incl, 63, 64);
        const int cnt = total < 64u ? (int)total : 64;
        uint32_t pos = incl - c;
#pragma unroll
        for (int i = 0; i < kB1Win; ++i) {
            if ((vis >> i) & 1u) {
                if (pos < 64u) {
                    lds.sidx[pos] = a0 + kB1Win * lane + i - range.x;
                    lds.smv[pos] = (wd >> (8 * i)) & 0xFu;
                    lds.sgd[pos] = gwa[i];
                }
                ++pos;
            }
        }
        __syncthreads();
        base = total > 64u ? (int)lds.sidx[63] + 1 : (int)(a0 + 64 * kB1Win - range.x);
        if (cnt == 0) {
            __syncthreads();
            continue;
        }
        uint32_t smask = 0;
        if (lane < cnt) {
            const uint32_t g = lds.sgd[lane];
            const uint4 rr = rect[g];
            const int minx = rr.x & 0xFFFF, miny = rr.x >> 16, maxx = rr.y & 0xFFFF;
            const int y0 = miny > geo.ty0 ? miny : geo.ty0;
            uint32_t jl = rr.z + (uint32_t)((ty - y0) * (maxx - minx) + (tx - minx));
            if (jl >= geo.cap) jl = 0xFFFFFFFFu;  // past the capacity: the entry is not written
            const float4* r = rec + 3 * (size_t)g;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            lds.srec[2 * lane] = r0;
            lds.srec[2 * lane + 1] = make_float4(r1.x, r2.w, __uint_as_float(jl), 0.0f);
            smask = lds.smv[lane];
        }
        __syncthreads();
        uint64_t todo = __ballot(lane < cnt);
        int visited = 0, parked = 0;
        while (todo) {
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r0 = lds.srec[2 * k], h = lds.srec[2 * k + 1];
            const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)smask, k) & live;
            const float dx = r0.x - pfx;
            const float bdx = r0.w * dx;
            const float K = fmaf(r0.z * dx, dx, h.y);
            float mx = 0.0f, sm = -0.f;  // -0: the identity of IEEE addition
            uint32_t np = 0;             // contributing pixels (scalar)
#pragma unroll
            for (int p = 0; p < SPW; ++p) {
                if (!(m & (1u << p))) continue;  // wave-uniform; exact: the stripe's pixels fail the alpha test
                const float dy = r0.y - pfy[p];
                const float e = fmaf(fmaf(h.x, dy, bdx), dy, K);
                float oG;
                bool keep;
                const float a = pair_alpha_keep(e, h.y, oG, keep);
                const float w = a * T[p];
                const float tT = T[p] - w;
                const bool ok = tT >= 0.0001f;
                const bool in = ok && keep;  // the pair is blended
                np += (uint32_t)__popcll(__ballot(in));
                const float wgt = in ? w : 0.0f;
                mx = fmaxf(mx, wgt);
                sm += wgt;
                T[p] = ok ? tT : -fabsf(T[p]);
            }
            if (np) {
                mx = fmaxf(mx, dpp_f<0xB1>(mx));  // quad_perm [1,0,3,2]
                sm += dpp_f<0xB1>(sm);
                mx = fmaxf(mx, dpp_f<0x4E>(mx));  // quad_perm [2,3,0,1]
                sm += dpp_f<0x4E>(sm);
                if ((lane & 3) == 0)
                    *reinterpret_cast<float2*>(lds.qpark + parked * kScSlot + (lane >> 2) * 2) = make_float2(mx, sm);
                if (lane == 0) lds.sjc[parked] = make_uint2(__float_as_uint(h.z), np);
                if (++parked == kScPark) {
                    flush(kScPark);
                    parked = 0;
                }
            }
            if ((++visited & 7) == 0) {
                uint32_t lv = 0;
#pragma unroll
                for (int p = 0; p < SPW; ++p) lv |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
                live = lv;
                if (live == 0) break;
            }
        }
        if (parked) flush(parked);
        __syncthreads();  // srec / the tables are rewritten by the next batch
    }
}

// Per-Gaussian combination of its entries [offsets[g - 1], offsets[g]) in entry order -- max, +,
// + -- the shape of gather_grad2d_kernel: a block owns 256 consecutive Gaussians, whose segments
// tile one stretch of the entry arrays, streamed through LDS in coalesced windows; unflagged
// entries count as (0, 0, 0) and are never loaded.  A culled Gaussian has no entries: 0, 0, 0.
// acc: the result is combined with what the output holds (max, +, +) instead of replacing it.
// rrect (presort mode): index i is a depth rank, its Gaussian rrect[i].z.
constexpr int kScoreWin = 512;

__global__ __launch_bounds__(256) void score_gather_kernel(const uint32_t* __restrict__ offsets, const ScoreOut in,
                                                           int P, uint32_t cap, const uint4* __restrict__ rrect,
                                                           float* __restrict__ max_w, float* __restrict__ sum_w,
                                                           uint32_t* __restrict__ hits, int acc) {
    __shared__ float wm[kScoreWin], ws[kScoreWin];
    __shared__ uint32_t wc[kScoreWin];
    const int g0 = blockIdx.x * 256, g = g0 + threadIdx.x;
    const int gl = (P - g0 < 256 ? P - g0 : 256) + g0;  // one past the block's last Gaussian
    // emission indices past the binning's capacity were never emitted (overflow): clamped
    auto off = [&](int i) { const uint32_t o = offsets[i]; return o < cap ? o : cap; };
    const uint32_t J0 = g0 ? off(g0 - 1) : 0u, J1 = off(gl - 1);
    const uint32_t s = g < P ? (g ? off(g - 1) : 0u) : 0u;
    const uint32_t e = g < P ? off(g) : 0u;
    float am = 0.0f, as = 0.0f;
    uint32_t ac = 0;
    for (uint32_t W = J0; W < J1; W += kScoreWin) {
        const uint32_t n = J1 - W < (uint32_t)kScoreWin ? J1 - W : (uint32_t)kScoreWin;
        static_assert(kScoreWin == 512, "two entries per thread");
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t i = threadIdx.x + 256u * k;
            if (i < n) {
                const bool on = in.fl[(size_t)W + i] != 0;
                wm[i] = on ? in.mx[(size_t)W + i] : 0.0f;
                ws[i] = on ? in.sm[(size_t)W + i] : 0.0f;
                wc[i] = on ? in.ct[(size_t)W + i] : 0u;
            }
        }
        __syncthreads();
        const uint32_t lo = s > W ? s : W, hi = e < W + n ? e : W + n;
        for (uint32_t j = lo; j < hi; ++j) {
            am = fmaxf(am, wm[j - W]);
            as += ws[j - W];
            ac += wc[j - W];
        }
        __syncthreads();
    }
    if (g >= P) return;
    const uint32_t gid = rrect ? rrect[g].z : (uint32_t)g;
    if (max_w) max_w[gid] = acc ? fmaxf(max_w[gid], am) : am;
    if (sum_w) sum_w[gid] = acc ? sum_w[gid] + as : as;
    if (hits) hits[gid] = acc ? hits[gid] + ac : ac;
}

ScoreOut score_arrays(void* scratch, long long cap) {
    const ScoreLayout sl(cap);
    return {at<float>(scratch, sl.mx), at<float>(scratch, sl.sm), at<uint32_t>(scratch, sl.ct),
            at<uint8_t>(scratch, sl.fl)};
}

}  // namespace

int launch_clear_score_flags(void* scratch, long long cap, hipStream_t s) {
    if (cap <= 0) return 0;
    return (int)hipMemsetAsync(at<uint8_t>(scratch, ScoreLayout(cap).fl), 0, (size_t)cap, s);
}

int launch_score_replay(const gsr_camera& cam, const uint2* ranges, const uint32_t* sorted_gid, const uint4* rect,
                        const float4* rec, void* scratch, long long cap, const uint32_t* term, const float4* ck,
                        const uint8_t* mk, hipStream_t s) {
    const float bg[3] = {0.0f, 0.0f, 0.0f};
    const BlendGeom geo = make_geo(cam, bg, 0, div_up(cam.height, kTile), cap, 0, 0);
    if (geo.nwg <= 0) return 0;
    const int blocks = 8 * (geo.nwg / 8 + 1) * kMaxChunks;  // B1's grid: one wave per (tile, chunk slot)
    hipLaunchKernelGGL(score_replay_kernel, dim3(blocks), dim3(64), 0, s, geo, ranges, sorted_gid, rect, rec,
                       score_arrays(scratch, cap), term, ck, mk);
    return (int)hipGetLastError();
}

int launch_score_gather(const uint32_t* offsets, void* scratch, long long cap, int P, const uint4* rrect,
                        float* max_w, float* sum_w, uint32_t* hits, bool accumulate, hipStream_t s) {
    if (P <= 0) return 0;
    hipLaunchKernelGGL(score_gather_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, offsets, score_arrays(scratch, cap),
                       P, (uint32_t)(cap > 0 ? cap : 0), rrect, max_w, sum_w, hits, accumulate ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace gsr
