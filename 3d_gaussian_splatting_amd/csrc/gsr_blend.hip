// gsr_blend.hip -- F6 per-tile front-to-back alpha blend and B1 per-tile front-to-back
// gradient pass on gfx950.
//
// Pixel layout: a 16x16 tile is four 16x4 stripes; lane l of a wave owns column l&15 and
// row (l>>4) of each stripe it covers.  F6 runs NW waves per tile (NW = 2 shipped: wave w
// owns stripes 2w, 2w+1); B1 runs one wave per tile (all four stripes, so each record's
// per-pixel terms are reduced once).  Batches of records are gathered one record per
// thread (3 dwordx4 loads), staged in LDS with a per-record stripe mask, and swept by every
// lane; a record whose alpha >= 1/255 footprint misses a stripe is skipped for that stripe
// by a wave-uniform branch (exact: the skipped pixels fail the alpha test).
//
// Both kernels are VALU-issue-bound (a wave64 VALU op costs 4 cycles of its SIMD, exp/rcp 8;
// MI355X_MICROARCH 'vector-instruction ISSUE cost'), so the per-(pixel, record) stream is
// kept short: log2(o) is folded into the exponent (o G = exp2(power + log2 o)), the
// column-only part of the quadratic form is hoisted per record, termination is encoded in
// the sign of T (no contributor count, no separate final-T register), and B1 accumulates
// per lane only the row moments (sum sv, sum sv dy, sum sv dy^2) -- the dx factors are
// applied once per record because dx is constant along a lane's column.
//
// Workgroup -> tile mapping is XCD-aware: blocks b, b+8, ... land on one XCD (observed
// round-robin dispatch, speed only), so each XCD gets a contiguous band of tile rows and
// its L2 keeps the records those neighbouring tiles share.
//
// B1 reduces each record's 9 raw moments over the tile's 256 pixels: 4 pixels per lane in
// registers, a 2-step quad DPP reduction, then the 16 quad partials wait in LDS and are summed
// four records at a time (one (record, moment) output per lane, stored straight to HBM) --
// ~40% fewer VALU ops than a full 64-lane DPP/permlane reduction per record, and no per-batch
// moment buffer in LDS (more waves per SIMD).  It writes ONE 36-B partial per contributing
// (tile, instance) with plain stores, indexed by the instance's emission index j, and sets that
// entry's flag byte; the gather reads flagged entries only (the launcher zeroes the K flag bytes,
// never the 36-B entries), and a tile stops at the first batch whose pixels have all terminated.
//
// Measured and rejected (experiments are separate builds,
// _build.build_variant + scripts/ab.sh): packing two stripes per VGPR pair (v_pk_fma_f32 issues
// 2 FMAs in 4 cycles -- no gain over v_fma_f32 on gfx950, and the register shuffles cost extra);
// 4 waves per tile; record prefetch into registers.  The per-Gaussian sum happens later in fixed
// emission order (gsr_preprocess_bwd.hip), so gradients are deterministic and no float atomics
// are issued.
#include "gsr_blend_dev.h"  // kPPL, xcd_tile, BlendGeom, pair_alpha: shared with gsr_scores.hip

namespace gsr {
namespace {

template <int CTRL>
__device__ inline float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

// Quad (4-lane) all-reduce of N values.  The empty asm pins each sum in the block that
// computes it: without it the compiler sinks the second add into the quad leaders' branch,
// the DPP move can no longer fuse into it, and each value costs a zero move, a DPP move and
// an add instead of one v_add_f32_dpp (2N extra VALU ops per record).
template <int N>
__device__ __forceinline__ void quad_reduce(float (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f<0xB1>(v[i]);  // quad_perm [1,0,3,2]
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f<0x4E>(v[i]);  // quad_perm [2,3,0,1]
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}



// Which of the tile's four 16x4 pixel stripes (slot p = rows 4p..4p+3) can hold a pixel
// with alpha >= 1/255.  Two conservative tests, both on the record the loading lane holds:
//  1. the padded footprint box (ext_x, ext_y) must overlap the stripe;
//  2. the footprint ellipse itself must reach the stripe's pixel-centre rectangle: with the
//     PD form Q(d) = -(a' dx^2 + b' dx dy + c' dy^2) (the exponent without log2 o), a pixel
//     passes alpha >= 1/255 iff Q <= log2(255 o), so the stripe is needed iff the minimum of Q
//     over the rectangle (0 if the mean is inside, else the minimum over its four edges,
//     each a clamped 1-D quadratic) is within that bound -- padded by 2 % + 0.05 for float
//     rounding.  Records whose form is not negative definite keep the box test only.
// Exact culling: a skipped stripe has no pixel that the per-pixel test would accept, so no
// output bit changes; the ellipse test removes ~22 % of the box test's stripe evaluations
// and ~17 % of the visited records at 1M/1080p (scripts/cull_stats.py).
// min over v in [v0, v1] of a u^2 + b u v + c v^2 (c > 0), given k = -b / (2c): the minimiser
// k u clamped to the edge.  k comes from a hardware reciprocal (1 ulp), not an IEEE division
// (~11 instructions each, 16 per record): a minimiser off by a few ulp raises q by c d^2, far
// inside the 2 % + 0.05 pad, and any point of the edge bounds the minimum from above only by
// that amount, so the test stays conservative.
__device__ __forceinline__ float edge_min_q(float a, float b, float c, float k, float u, float v0, float v1) {
    const float vs = fminf(fmaxf(k * u, v0), v1);
    return fmaf(fmaf(c, vs, b * u), vs, a * u * u);
}

__device__ inline uint32_t stripe_mask(const float4 r0, const float4 r1, const float4 r2, float bx0, float by0) {
    const float ex = r2.y, ey = r2.z;
    if (!(ex >= 0.0f) || r0.x + ex < bx0 || r0.x - ex > bx0 + 15.0f) return 0u;
    const float ylo = r0.y - ey, yhi = r0.y + ey;
    // PD form coefficients (A dx^2 + B dx dy + C dy^2) and the log2-domain bound
    const float A = -r0.z, B = -r0.w, C = -r1.x;
    const bool pd = A > 0.0f && C > 0.0f && 4.0f * A * C - B * B > 0.0f;
    const float bound = fmaf(fmaxf(r2.w + 7.99435343f, 0.0f), 1.02f, 0.05f);  // log2(255 o)
    const float x0 = bx0 - r0.x, x1 = bx0 + 15.0f - r0.x;  // rect in mean-relative coords
    const float kc = -B * __builtin_amdgcn_rcpf(2.0f * C), ka = -B * __builtin_amdgcn_rcpf(2.0f * A);
    uint32_t m = 0;
#pragma unroll
    for (int p = 0; p < kPPL; ++p) {
        const float s0 = by0 + 4.0f * p;
        bool hit = yhi >= s0 && ylo <= s0 + 3.0f;
        if (hit && pd) {
            const float y0 = s0 - r0.y, y1 = s0 + 3.0f - r0.y;
            const bool inside = x0 <= 0.0f && x1 >= 0.0f && y0 <= 0.0f && y1 >= 0.0f;
            const float q = fminf(fminf(edge_min_q(A, B, C, kc, x0, y0, y1), edge_min_q(A, B, C, kc, x1, y0, y1)),
                                  fminf(edge_min_q(C, B, A, ka, y0, x0, x1), edge_min_q(C, B, A, ka, y1, x0, x1)));
            hit = inside || q <= bound;
        }
        m |= hit ? (1u << p) : 0u;
    }
    return m;
}

// B1 chunk size in (record, stripe) pairs it will visit (see kMaxChunks).  One pair is one
// 64-lane evaluation in B1; a tile's front 48 records with four live stripes are 192.  Measured
// at 1M / 1080p (B1 ms, F6 WRITE_SIZE MB incl. 58 MB of image): 128: 0.467, 187; 192: 0.466,
// 175; 256: 0.473, 141; 384: 0.481, ~115; 512: 0.501, 100; 768: 0.526, 87.  F6's time does not
// move with its checkpoint writes (0.253-0.259 ms across the range: they overlap the blend),
// B1's does, so the bound is set for B1.  At 5M / 1080p: 128: 0.488, 256: 0.492, 512: 0.524.
// (kChunkWork / GSR_CHUNK_WORK and the band launches' GSR_BAND_CHUNK_WORK: gsr_internal.h)

// F6.  T > 0: pixel live; T <= 0: done, |T| = final transmittance (the T after the last
// contributor -- the reference's final_T).  A pair is blended when the next transmittance
// T - alpha T (the reference's T (1 - alpha), one op shorter) is >= 1e-4; otherwise the pixel
// terminates with T unchanged (SURVEY B.3 / forward.cu renderCUDA).  The exponent is
// Horner-form: ((c' dy + b' dx) dy) + (a' dx^2 + log2 o), 3 ops per stripe with dy.
// records per batch of the four-wave (band) F6: one per thread (128: four waves sharing the
// two-wave kernel's 128-record batches)
constexpr int kF6Batch4 = 256;
// two-wave (full-image) F6 held to 8 waves per SIMD (64 VGPRs): the gid-ahead register would
// otherwise take it to 65 and 7 waves
constexpr int kF6Wpe = 8;
// Depth / alpha channel (gsr_forward_aux, gsr_backward_aux).  The aux variants of F6 and B1 are the
// same kernels instantiated with one more trailing argument (the pack AX = {F6Aux} / {B1Aux}); with
// the pack empty every `if constexpr (AUX)` block drops out and the kernel -- arguments, registers,
// LDS, instructions -- is the plain one.  v_i, the value the channel blends, is the Gaussian's
// view-space depth (the float whose bits are its depth key) or its reciprocal; it is staged in LDS
// beside the record at batch load (the 48-byte record has no free lane).
template <class T>
__device__ __forceinline__ T aux_arg() { return T{}; }
template <class T>
__device__ __forceinline__ T aux_arg(const T& a) { return a; }
__device__ __forceinline__ float aux_value(uint32_t key, int inv) {
    const float z = __uint_as_float(key);
    return inv ? 1.0f / z : z;
}
// The aux F6 variants hold one more accumulator per pixel: kF6AuxWpe waves per SIMD for the
// two-wave form (DESIGN.md "Depth and alpha outputs" has the compiler's resource report)
constexpr int kF6AuxWpe = 7;
template <int NW, class... AX>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 2 ? (sizeof...(AX) ? kF6AuxWpe : kF6Wpe) : 1))) void blend_forward_kernel(const BlendGeom geo,
                                                                const uint2* __restrict__ ranges,
                                                                const uint32_t* __restrict__ sorted_gid,
                                                                const float4* __restrict__ rec,
                                                                float* __restrict__ out_color,
                                                                float* __restrict__ final_T,
                                                                float* __restrict__ accum,
                                                                uint32_t* __restrict__ term,
                                                                float4* __restrict__ ck,
                                                                uint8_t* __restrict__ mk, const AX... axp) {
    constexpr bool AUX = sizeof...(AX) > 0;
    static_assert(sizeof...(AX) <= 1, "one aux argument");
    const F6Aux ax = aux_arg<F6Aux>(axp...);
    constexpr int PPL = kPPL / NW;
    // records per batch: one per thread
    constexpr int BATCH = NW > 2 ? kF6Batch4 : 64 * NW;
    static_assert(BATCH % 64 == 0 && BATCH <= 64 * NW, "F6 batch");
    constexpr int kCW = NW > 2 ? kBandChunkWork : kChunkWork;
    __shared__ float4 srec[BATCH * 3];
    __shared__ uint32_t smk[BATCH];
    __shared__ uint32_t slive[NW];
    __shared__ float svz[AUX ? BATCH : 1];  // aux: the batch's v_i (unused, so absent, otherwise)
    const int tl = xcd_tile(blockIdx.x, geo.nwg);  // band-local tile index
    const int tile = tl + geo.ty0 * geo.grid_x;
    const int tx = tile % geo.grid_x, ty = tile / geo.grid_x;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int px = tx * kTile + (lane & 15);
    const float pfx = (float)px;
    const int view = ty / geo.vgy, tyl = ty - view * geo.vgy;  // tile row inside its view's band
    const float bx0 = (float)(tx * kTile), by0 = (float)(tyl * kTile);
    float pfy[PPL], T[PPL], C0[PPL], C1[PPL], C2[PPL];
    float Z[PPL];  // aux: sum w v
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const int pyl = tyl * kTile + (lane >> 4) + 4 * (w * PPL + p);
        pfy[p] = (float)pyl;
        T[p] = (px < geo.W && pyl < geo.vh) ? 1.0f : -1.0f;
        C0[p] = C1[p] = C2[p] = 0.0f;
        Z[p] = 0.0f;
    }
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    // aux: the depth channel is accumulated relative to vref, the value of the tile's first (nearest)
    // record: Zc = sum w (v - vref), depth = Zc + vref (1 - T_final).  A pixel's values differ little
    // along its depth-sorted list, so the f32 sum then rounds at the size of the depth spread, not of
    // the depth -- B1 replays the sum as a running difference and inherits its rounding error whole.
    float vref = 0.0f;
    if constexpr (AUX) {
        if (n > 0) vref = aux_value(ax.depth_key[sorted_gid[range.x]], ax.inv);
    }
    // B1 chunk checkpoints: (T, colour sum) of every pixel where a chunk starts.  `work` counts
    // the (record, stripe) pairs of the current chunk: a record's stripe mask against the stripes
    // live (anywhere in the tile) at the start of its batch -- block-uniform, so every wave takes
    // the same chunk decisions, including a wave whose own pixels have all finished (it keeps
    // writing its final state at the later checkpoints).
    uint32_t* const table = term + (size_t)tl * kMaxChunks;  // [term, chunk 1.. starts]
    int nck = 0;   // checkpoints written
    int work = 0;  // pairs in the current chunk
    int tend = n;  // termination index: every pixel of the tile has finished before record tend
    // A stripe with no live pixel (its `live` bit clear: conservative, the bit is cleared only
    // once every T <= 0) is not written; its byte tells B1 to start it dead (T = -1), which is
    // all B1 needs of a finished pixel.
    uint8_t* const ckm = reinterpret_cast<uint8_t*>(ck + (size_t)geo.ck_slots * 256);
    auto checkpoint = [&](size_t slot, uint32_t lv) {
        float4* dst = ck + (size_t)slot * 256;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const bool on = (lv >> p) & 1u;  // wave-uniform
            if (on) dst[64 * (w * PPL + p) + lane] = make_float4(T[p], C0[p], C1[p], C2[p]);
            if constexpr (AUX) {
                if (on) ax.ckz[(size_t)slot * 256 + 64 * (w * PPL + p) + lane] = Z[p];
            }
            if (lane == 0) ckm[4 * (size_t)slot + w * PPL + p] = on ? 1 : 0;
        }
    };
    // Chunk merging.  When all kMaxChunks - 1 chunk starts are taken and the current chunk is
    // full, neighbouring chunks are merged pairwise (the even starts are kept: chunk k of the
    // merged table is chunk 2k of the old one, its checkpoint moved to slot k) and the quota
    // doubles, so B1's chunks stay within ~2x of each other in work however long the list --
    // without it the last chunk of a deep tile takes all the remaining work (after an opacity
    // reset nothing terminates: 624 of 4160 tiles at 6M / 1280x832 had a 50k-entry last chunk,
    // B1 7.9 ms of a 15.6 ms iteration).  Each thread moves exactly the checkpoint words it
    // wrote (same index map as `checkpoint`), and slot k is read (as the source of k / 2)
    // before it is overwritten, so the moves need no barrier.
    int quota = kCW;
    auto merge_chunks = [&]() {
        constexpr int kKeep = (kMaxChunks - 1) / 2;
        // a tile's chunk slots are consecutive in both layouts: chunk c at ck_slot_of(.., 1) + c - 1
        float4* const ckt = ck + ck_slot_of(geo.ck_fixed, range.x, tl, 1) * 256 - 256;
        uint8_t* const ckmt = ckm + (ck_slot_of(geo.ck_fixed, range.x, tl, 1) - 1) * 4;
#pragma unroll 1
        for (int k = 1; k <= kKeep; ++k) {
#pragma unroll 1
            for (int p = 0; p < PPL; ++p) {
                const int i = 64 * (w * PPL + p) + lane;
                ckt[256 * k + i] = ckt[512 * k + i];
                if constexpr (AUX) {  // the slot's depth words move with it
                    float* const ckzt = ax.ckz + ck_slot_of(geo.ck_fixed, range.x, tl, 1) * 256 - 256;
                    ckzt[256 * k + i] = ckzt[512 * k + i];
                }
                if (lane == 0) ckmt[4 * k + w * PPL + p] = ckmt[8 * k + w * PPL + p];
            }
            if (tid == 0) table[k] = table[2 * k];
        }
        nck = kKeep;
        work += quota;  // the merged current chunk: old chunk 2 kKeep (>= one quota) + the open one
        quota *= 2;
    };
    // each batch's gid is loaded one batch ahead (one VGPR), so a batch start waits for its record
    // loads only, not for the gid load they depend on as well
    uint32_t g_next = tid < BATCH && tid < n ? sorted_gid[range.x + tid] : 0u;
    for (int base = 0; base < n; base += BATCH) {
        uint32_t live = 0;
#pragma unroll
        for (int p = 0; p < PPL; ++p) live |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
        if (lane == 0) slive[w] = live << (w * PPL);
        if (tid < BATCH && base + tid < n) {
            const uint32_t g = g_next;
            if (base + BATCH + tid < n) g_next = sorted_gid[range.x + base + BATCH + tid];
            const float4* r = rec + 3 * (size_t)g;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            srec[3 * tid + 0] = r0;
            srec[3 * tid + 1] = r1;
            srec[3 * tid + 2] = r2;
            smk[tid] = stripe_mask(r0, r1, r2, bx0, by0);
            if constexpr (AUX) svz[tid] = aux_value(ax.depth_key[g], ax.inv) - vref;
            mk[range.x + base + tid] = (uint8_t)smk[tid];  // B1's visit filter
        } else if (tid < BATCH) {
            smk[tid] = 0u;
        }
        __syncthreads();
        uint32_t tile_live = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) tile_live |= slive[i];
        // termination from the batch barrier's own slive words (__syncthreads_or is three
        // barriers); the batch just loaded is then discarded, and its mask bytes lie at or past
        // tend, where B1 never reads
        if (tile_live == 0) {
            tend = base;
            break;
        }
        const int cnt = (n - base) < BATCH ? (n - base) : BATCH;
        int visited = 0;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const uint32_t sm = smk[c0 + lane];  // 0 past cnt
            // at the group boundary where a 32nd chunk would open
            if (__builtin_expect(work >= quota && nck == kMaxChunks - 1, 0)) merge_chunks();
            if (work >= quota && nck < kMaxChunks - 1) {  // chunk nck + 1 starts at base + c0
                ++nck;
                checkpoint(ck_slot_of(geo.ck_fixed, range.x, tl, nck), live);
                if (tid == 0) table[nck] = (uint32_t)(base + c0);
                work = 0;
            }
            const uint32_t tm = sm & tile_live;
            work += __popcll(__ballot(tm & 1u)) + __popcll(__ballot(tm & 2u)) + __popcll(__ballot(tm & 4u)) +
                    __popcll(__ballot(tm & 8u));
            if (!live) continue;
            const uint32_t mine = (sm >> (w * PPL)) & ((1u << PPL) - 1u);
            uint64_t todo = __ballot((mine & live) != 0u && c0 + lane < cnt);
            // Band launches (NW = 4: one stripe per wave, every block resident at once) are bound
            // by one wave's dependent chain per record, not by issue: there two records are taken
            // per pass -- both alphas first (they do not depend on T), then the T / colour
            // updates in list order, so the result is bit-identical.
            if constexpr (PPL == 1) {
                while (todo) {
                    const int ka = c0 + __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const bool two = todo != 0;  // wave-uniform
                    const int kb = two ? c0 + __builtin_ctzll(todo) : ka;
                    if (two) todo &= todo - 1;
                    const float4 a0 = srec[3 * ka + 0], a1 = srec[3 * ka + 1], a2 = srec[3 * ka + 2];
                    const float4 b0 = srec[3 * kb + 0], b1 = srec[3 * kb + 1], b2 = srec[3 * kb + 2];
                    const float dxa = a0.x - pfx, dxb = b0.x - pfx;
                    const float dya = a0.y - pfy[0], dyb = b0.y - pfy[0];
                    const float ea = fmaf(fmaf(a1.x, dya, a0.w * dxa), dya, fmaf(a0.z * dxa, dxa, a2.w));
                    const float eb = fmaf(fmaf(b1.x, dyb, b0.w * dxb), dyb, fmaf(b0.z * dxb, dxb, b2.w));
                    float oGa, oGb;
                    const float aa = pair_alpha(ea, a2.w, oGa);
                    const float ab = pair_alpha(eb, b2.w, oGb);
                    {
                        const float w = aa * T[0];
                        const float tT = T[0] - w;
                        const bool ok = tT >= 0.0001f;
                        const float wgt = ok ? w : 0.0f;
                        C0[0] = fmaf(a1.z, wgt, C0[0]);
                        C1[0] = fmaf(a1.w, wgt, C1[0]);
                        C2[0] = fmaf(a2.x, wgt, C2[0]);
                        if constexpr (AUX) Z[0] = fmaf(svz[ka], wgt, Z[0]);
                        T[0] = ok ? tT : -fabsf(T[0]);
                    }
                    if (two) {
                        const float w = ab * T[0];
                        const float tT = T[0] - w;
                        const bool ok = tT >= 0.0001f;
                        const float wgt = ok ? w : 0.0f;
                        C0[0] = fmaf(b1.z, wgt, C0[0]);
                        C1[0] = fmaf(b1.w, wgt, C1[0]);
                        C2[0] = fmaf(b2.x, wgt, C2[0]);
                        if constexpr (AUX) Z[0] = fmaf(svz[kb], wgt, Z[0]);
                        T[0] = ok ? tT : -fabsf(T[0]);
                    }
                    const int before = visited;
                    visited += two ? 2 : 1;
                    if ((before >> 3) != (visited >> 3)) {
                        live = __any(T[0] > 0.0f) ? 1u : 0u;
                        if (live == 0) break;
                    }
                }
                continue;
            }
            while (todo) {
                const int kk = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int k = c0 + kk;
                const float4 r0 = srec[3 * k + 0];
                const float4 r1 = srec[3 * k + 1];
                const float4 r2 = srec[3 * k + 2];
                const float dx = r0.x - pfx;
                const float bdx = r0.w * dx;
                const float K = fmaf(r0.z * dx, dx, r2.w);  // column part of the exponent + log2 o
                float vz = 0.0f;
                if constexpr (AUX) vz = svz[k];
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    // No per-stripe branch: a culled stripe's pixels all get alpha 0 (exact test),
                    // which leaves C and T bit-for-bit unchanged, and with two waves per tile both
                    // stripes of a visited record run in one basic block -- the two chains
                    // interleave (0.257 vs 0.263 ms with the branch; with four waves a visited
                    // record always covers the wave's one stripe).  B1 keeps the branch (its
                    // culled stripes skip 28 ops, branchless 0.518 vs 0.465 ms).
                    const float dy = r0.y - pfy[p];
                    const float e = fmaf(fmaf(r1.x, dy, bdx), dy, K);
                    float oG;
                    const float a = pair_alpha(e, r2.w, oG);
                    const float w = a * T[p];
                    const float tT = T[p] - w;
                    const bool ok = tT >= 0.0001f;
                    const float wgt = ok ? w : 0.0f;
                    C0[p] = fmaf(r1.z, wgt, C0[p]);
                    C1[p] = fmaf(r1.w, wgt, C1[p]);
                    C2[p] = fmaf(r2.x, wgt, C2[p]);
                    if constexpr (AUX) Z[p] = fmaf(vz, wgt, Z[p]);
                    T[p] = ok ? tT : -fabsf(T[p]);
                }
                if ((++visited & 7) == 0) {
                    uint32_t lv = 0;
#pragma unroll
                    for (int p = 0; p < PPL; ++p) lv |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
                    live = lv;
                    if (live == 0) break;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        table[0] = (uint32_t)tend;
        for (int c = nck + 1; c < kMaxChunks; ++c) table[c] = 0xFFFFFFFFu;
    }
    // per view: [3, vh, W] colour planes and a [vh, W] transmittance plane (one image: view 0)
    const size_t npix = (size_t)geo.W * geo.vh;
    float* const oc = out_color + (size_t)view * 3 * npix;
    float* const ac = accum + (size_t)view * 3 * npix;
    float* const fT = final_T + (size_t)view * npix;
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        // the row back from its float (exact: a small integer), so that the integer does not stay
        // live through the visit loop -- with it live, the 64-VGPR cap of kF6Wpe has pfy[0]
        // converted again on every visit
        const int pyl = (int)pfy[p];
        if (px < geo.W && pyl < geo.vh) {
            const size_t pix = (size_t)pyl * geo.W + px;
            const float Tf = fabsf(T[p]);
            fT[pix] = Tf;
            ac[pix] = C0[p];
            ac[npix + pix] = C1[p];
            ac[2 * npix + pix] = C2[p];
            oc[pix] = C0[p] + Tf * geo.bg0;
            oc[npix + pix] = C1[p] + Tf * geo.bg1;
            oc[2 * npix + pix] = C2[p] + Tf * geo.bg2;
            if constexpr (AUX) {  // one image (aux launches have no views): no background term
                ax.accum_z[pix] = Z[p];  // centred (B1 takes the same vref)
                ax.out_depth[pix] = fmaf(vref, 1.0f - Tf, Z[p]);
                ax.out_alpha[pix] = 1.0f - Tf;
            }
        }
    }
}

// A record as B1 stages it in LDS: the 9 floats its record loop reads (kStagedRec floats a row)
constexpr int kStagedRec = 10;
struct StagedRec {
    float4 r0;  // mean x, y, conic a (scaled), b
    float4 h;   // r1.x, r1.z, r1.w, r2.x
    float L;    // r2.w
};
__device__ __forceinline__ StagedRec staged(const float2* srec, int k) {
    const float2* p = srec + k * (kStagedRec / 2);
    const float2 a = p[0], b = p[1], c = p[2], d = p[3];
    return {make_float4(a.x, a.y, b.x, b.y), make_float4(c.x, c.y, d.x, d.y), p[4].x};
}

// Deferred B1 reduction.  A record's 9 per-lane moments are quad-reduced by DPP; the 16 quad
// partials wait in LDS, and every kPark records one (record, moment) output per lane is summed
// from LDS in fixed quad order (four chains over quad & 3, then (t0 + t1) + (t2 + t3): the sum
// does not depend on kPark or on which lane takes it) and stored straight to the partial arrays
// at the record's emission index j (8 moments in part8[2j..2j+1], the 9th in part1[j]).
// Depth 4: at 5 (one more slot, 6,640 B of LDS) the flush's share of a record falls from 5.3 to
// 4.2 VALU, but B1 loses the occupancy it has at 5,760 B and is slower (0.4485 vs 0.4268 ms at
// 1M / 1080p).
constexpr int kPark = 4;
// Parking slot stride and the flush's lane map.  The flush reads with ds_read_b32, whose banks
// are (address / 4) mod 32 over lane groups {0-31}, {32-63} (MI355X_MICROARCH.md, LDS table).
// The flush lane of (slot s, moment c) reads word s kParkSlot + c + 12 i for quad i, so within a
// lane group the words s kParkSlot + c must differ mod 32.  The stride is a multiple of 4 (the
// leaders' float4 stores), so slot s covers the 9 (aux: 10) banks from 4 (m s mod 8), m =
// kParkSlot / 4: three slots that start 4 and 8 banks apart put three lanes on one bank, which two
// lane groups cannot separate.  Four slots take m = 2 (starts 0, 8, 16, 24: stride 200 = 16 quads
// x 12 floats + 8); five take m = 3 (starts 0, 12, 24, 4, 16: stride 204), every bank under at
// most two slots; 6 or 7 slots always hold such a triple, so this row allows no more than 5.
// make_flush_map deals the (slot, moment) pairs to the two lane groups, first fit by bank, and the
// static assertions hold the result to the rule: no two lanes of a group on one bank.
// Round 4's map (s = l / 9, c = l mod 9, stride 204) ignored the groups and put slots 2 / 3 on
// slot 0's banks: a 2-way conflict on every flush read, the ~9.5e6 SQ_LDS_BANK_CONFLICT cycles per
// launch of profiles/r04_pmc_summary.txt (16 reads x ~6.3e5 flushes at 1M / 1080p).
constexpr int kParkSlot = 16 * 12 + (kPark <= 4 ? 8 : 12);
static_assert(kPark <= 5 && kParkSlot % 4 == 0, "flush banks / float4 alignment of the leaders' stores");
struct FlushMap {
    uint8_t sc[64];  // per flush lane: slot << 4 | moment, 0xFF for an idle lane
    bool ok;
};
constexpr FlushMap make_flush_map(int moments) {
    FlushMap m{};
    for (int l = 0; l < 64; ++l) m.sc[l] = 0xFF;
    m.ok = true;
    bool used[2][32] = {};
    int fill[2] = {0, 0};
    for (int s = 0; s < kPark; ++s)
        for (int c = 0; c < moments; ++c) {
            const int bank = (s * kParkSlot + c) % 32;
            const int g = used[0][bank] ? 1 : 0;
            if (used[g][bank] || fill[g] == 32) {
                m.ok = false;
                continue;
            }
            used[g][bank] = true;
            m.sc[32 * g + fill[g]++] = (uint8_t)(s << 4 | c);
        }
    return m;
}
__device__ constexpr FlushMap kFlushMap = make_flush_map(9), kFlushMapAux = make_flush_map(10);
static_assert(kFlushMap.ok && kFlushMapAux.ok, "flush lanes of one group on one LDS bank");
// The parked records' batch indices ride in one scalar word (6 bits per slot: `kpack`); the
// flush lane of slot s reads its record's emission index from the record's staged row (its tenth
// word, written once per batch), so a record costs no per-record readlane / LDS write for it.
static_assert(6 * kPark <= 32, "kpack");
// AUX: a tenth moment (row slot 9) goes to its own per-entry array pz.
// A flush lane's slot, moment and destination are fixed for the whole kernel (FlushLane, set at
// kernel start): the LDS address of its first quad partial, and a base and byte step into its
// moment's home array (part8 + c floats and 32 B per entry for c < 8, part1 or pz and 4 B
// otherwise), so an entry's address is one multiply-add from j per flush.
typedef const __attribute__((address_space(3))) float* LdsFloats;
struct FlushLane {
    // qpark + slot * kParkSlot + moment, as an LDS address the compiler cannot see into: the 16
    // reads are then immediate offsets from this one register (from qpark's known offset in the
    // LDS block it derives up to three bases, an add each per flush)
    LdsFloats q;
    char* base;
    uint32_t step;
    int slot;        // kPark for an idle lane: never below `parked`
    bool flag;       // moment 8 sets the entry's flag byte
};
template <bool AUX = false>
__device__ __forceinline__ FlushLane flush_lane(int lane, const float* qpark, float* p8f, float* p1, float* pz) {
    const int sc = AUX ? kFlushMapAux.sc[lane] : kFlushMap.sc[lane];
    const int c = sc & 15, slot = sc == 0xFF ? kPark : sc >> 4;
    float* b = c < 8 ? p8f + c : p1;
    if constexpr (AUX) b = c == 9 ? pz : b;
    LdsFloats q = (LdsFloats)(qpark + (sc == 0xFF ? 0 : slot * kParkSlot + c));
    asm volatile("" : "+v"(q));
    return {q, reinterpret_cast<char*>(b), c < 8 ? 32u : 4u, slot, c == 8};
}
__device__ __forceinline__ void park_flush(const FlushLane f, const float2* srec, uint32_t kpack, int parked,
                                           uint8_t* fl) {
    __syncthreads();  // one-wave block: orders the quad leaders' LDS writes before the reads
    if (f.slot < parked) {
        // -0 is the identity of IEEE addition, so the first add of each chain folds into a move
        float t[4] = {-0.f, -0.f, -0.f, -0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i & 3] += f.q[i * 12];
        const uint32_t j = __float_as_uint(srec[((kpack >> (6 * f.slot)) & 63u) * (kStagedRec / 2) + 4].y);
        if (j != 0xFFFFFFFFu) {  // an entry past the capacity (binning overflow) has none
            *reinterpret_cast<float*>(f.base + (size_t)j * f.step) = (t[0] + t[1]) + (t[2] + t[3]);
            if (f.flag) fl[j] = 1;  // the gather reads flagged entries only
        }
    }
    __syncthreads();
}

// B1 front to back.  With S = the forward's colour sum (no background) and the running
// Sp = sum over processed contributors of w * (c . dL/dpix), the colour behind entry k is
// (S . dL/dpix - Sp) / (1 - alpha_k) after T_k, so
//   dL/dalpha_k = T_k (c_k . dL/dpix) - R / (1 - alpha_k),
//   R = S . dL/dpix + T_final bg . dL/dpix - Sp
// (SURVEY B.4 rewritten; same value as the back-to-front recursion).  A lane keeps R itself
// (R -= w (c . dL/dpix) per contributor), one register and one op fewer than Sp and S.  T is
// recomputed with the forward's own instructions (same exponent, alpha, T - alpha T and sign
// encoding), so
// the set of contributing pairs -- and the termination point -- is exactly the forward's.
// Per record the lane accumulates sv = o G dL/dalpha moments along its column
// (sum sv, sum sv dy, sum sv dy^2) and applies dx afterwards:
//   Sx = dx sum sv, Sxx = dx^2 sum sv, Sxy = dx sum sv dy.
// B1 stores the raw tile sums (Sx, Sy, Sxx, Sxy, Syy, S0, colour x3); they are linear in the
// gradients, so gather_grad2d converts them once per Gaussian after summing over tiles.
//
// Batches: F6 stores the stripe mask of every list entry it loads (one byte each, `mk`); B1 reads
// 256 of them per step (one aligned word per lane), keeps the entries with a stripe still live
// and takes up to 64 of them, in list order, as its batch -- records that cannot touch a live
// stripe are never loaded (after an opacity reset most of a deep list is culled this way).
// Grid: one 64-lane block per (tile, chunk slot); chunk c > 0 starts where F6's chunk table
// says and resumes from F6's checkpoint, and slots the tile has no chunk for exit at once.  Each
// XCD (blocks b with equal b % 8) takes a contiguous tile range as in xcd_tile, visited
// chunk-major, so every tile's first chunk is dispatched first.
// 6 waves per SIMD: 78 VGPRs (no spills) and 5,760 B of LDS per one-wave block (2,560 staged
// records + 3,200 parking; the aux form's svz makes it 6,016 B, under its own 5-wave cap).
// Rounds 4 and 6 had let the block grow to 7,296 B with three batch tables: 22 blocks per 160-KiB
// CU, 5.5 waves per SIMD, not the 6 the registers allow.  The tables now share the parking area's
// bytes, the staged record lost the three floats the loop never reads, and the emission index took
// the row's spare word.  6,528 B (the shared tables alone) did not bring the occupancy back,
// 5,760 B did: B1 0.447 against 0.427 ms with the same instructions, so
// the block must stay well under 160 KiB / 24.  Measured (round 1) 0.552 ms vs 0.564 at the
// compiler's own 85 VGPRs (5 waves); 7 and 8 waves spill.
// kB1Win (gsr_internal.h) mask bytes per lane in one batch window: 256 entries per window.  B1
// loads the window's gids with its mask bytes (one 16-B load per lane), so a batch's record
// loads do not wait on a gid load first.
// One wave per (tile, chunk) owns the tile's four 16x4 stripes and writes one partial entry per
// (tile, instance).
// PF (band launches): each visited record's LDS reads are issued before the
// previous record's work (2x unrolled, no register copies) -- with ~3 one-wave blocks per SIMD on a
// band's 1020 tiles the LDS latency per record is exposed, where on full images other waves hide
// it (round 4: the same prefetch at full occupancy measured 0.456 vs 0.447 ms).
// The aux B1 variants keep dL/ddepth per pixel and a tenth moment: kB1AuxWpe
// waves per SIMD (DESIGN.md "Depth and alpha outputs")
constexpr int kB1AuxWpe = 5;
template <bool PF = false, class... AX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PF ? 4 : (sizeof...(AX) ? kB1AuxWpe : 6)))) void blend_backward_kernel(const BlendGeom geo,
                                                            const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ sorted_gid,
                                                            const uint4* __restrict__ rect,
                                                            const float4* __restrict__ rec,
                                                            const float* __restrict__ final_T,
                                                            const float* __restrict__ accum,
                                                            const float* __restrict__ dL_dpix,
                                                            float* __restrict__ p8f,
                                                            float* __restrict__ p1,
                                                            uint8_t* __restrict__ fl,
                                                            const uint32_t* __restrict__ term,
                                                            const float4* __restrict__ ck,
                                                            const uint8_t* __restrict__ mk, const AX... axp) {
    constexpr bool AUX = sizeof...(AX) > 0;
    static_assert(sizeof...(AX) <= 1, "one aux argument");
    constexpr int SPW = kPPL;  // the wave's stripes: all of the tile's
    const B1Aux ax = aux_arg<B1Aux>(axp...);
    __shared__ float svz[AUX ? 64 : 1];  // aux: the batch's v_i (unused, so absent, otherwise)
    // One block of LDS with srec first: the record fields then sit within the immediate offsets
    // of the record reads (8-bit offsets of ds_read2), so a record costs no address add.  A staged
    // record is the 9 floats the record loop reads in a 40-B row (8-B aligned for ds_read2_b64):
    // r0, then (r1.x, r1.z, r1.w, r2.x), then r2.w -- not the 12 of the global record -- and in the
    // row's tenth word the entry's emission index, which the flush lanes read by batch slot.
    __shared__ struct {
        float2 srec[64 * kStagedRec / 2];
        // The batch selection's tables share qpark's bytes: they are written and read back before
        // the batch's first record is parked, and rewritten after its last flush (one wave, whose
        // LDS operations complete in program order)
        union {
            float qpark[kPark * kParkSlot];  // [slot][quad][9 of 12]
            struct {
                uint32_t sidx[64];           // the batch's entries (list offsets), in list order
                uint32_t smv[64];            // and their stripe masks
                uint32_t sgd[64];            // and their gids (loaded with the window's mask bytes)
            };
        };
    } lds;
    float2* const srec = lds.srec;
    float* const qpark = lds.qpark;
    const int lane = threadIdx.x;
    float* const qlane = qpark + (lane >> 2) * 12;  // this quad's parking row
    int tl, chunk;
    {
        const int q = geo.nwg / 8, r = geo.nwg % 8, xcd = blockIdx.x % 8, local = (int)(blockIdx.x / 8);
        const int t0 = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, nt = q + (xcd < r ? 1 : 0);
        const int per = q + 1;  // padded tiles per XCD
        chunk = local / per;
        const int i = local - chunk * per;
        if (i >= nt) return;
        tl = t0 + i;
    }
    const int tile = tl + geo.ty0 * geo.grid_x;
    const uint2 range = ranges[tile];
    const int n_all = (int)(range.y - range.x);
    // F6's chunk table: [termination index, chunk 1..kMaxChunks-1 starts (UINT32_MAX: none)]
    const uint32_t* table = term + (size_t)tl * kMaxChunks;
    const uint32_t tend = table[0];
    const uint32_t start_u = chunk == 0 ? 0u : table[chunk];
    // no such chunk for this tile, or every pixel had finished before it
    if (start_u >= (uint32_t)n_all || start_u >= tend) return;
    const int start = (int)start_u;
    float vref = 0.0f;  // aux: F6's centre of the tile's depth values (its first record's)
    if constexpr (AUX) vref = aux_value(ax.depth_key[sorted_gid[range.x]], ax.inv);
    const uint32_t next = chunk + 1 < kMaxChunks ? table[chunk + 1] : 0xFFFFFFFFu;
    const int n = next < (uint32_t)n_all ? (int)next : n_all;
    const int tx = tile % geo.grid_x, ty = tile / geo.grid_x;
    // lane = 4 col + row: a quad holds one column's 4 rows of a stripe, so it shares dx and
    // the record's moments reduce over the quad before dx is applied (F6 lays a stripe out
    // row-major, lane = col + 16 row; B1 reads F6's checkpoints through that map)
    const int col = lane >> 2, row = lane & 3;
    const int px = tx * kTile + col;
    const float pfx = (float)px;
    const int view = ty / geo.vgy, tyl = ty - view * geo.vgy;  // tile row inside its view's band
    // F6's per-view planes (one image: view 0)
    const size_t npix = (size_t)geo.W * geo.vh;
    final_T += (size_t)view * npix;
    accum += (size_t)view * 3 * npix;
    dL_dpix += (size_t)view * 3 * npix;
    // R = S . dL/dpix - Sp + T_final bg . dL/dpix: the colour term behind the current record
    float pfy[SPW], T[SPW], R[SPW], dp0[SPW], dp1[SPW], dp2[SPW];
    // aux: dL/ddepth of the pixel, and v0 = its alpha-weighted mean of the (vref-centred) depth values.
    // The depth channel is replayed centred on vref + v0: sum_{j>k} w_j v_j = sum_{j>k} w_j (v_j - v0) + v0 (T_{k+1} - T_final) for
    // any constant v0, so with v'_j = v_j - v0 the channel is a colour v' over a background -v0
    //   dL/dalpha_k (depth) = dpz (T_k v'_k - (sum_{j>k} w_j v'_j - v0 T_final) / (1 - alpha_k)).
    // R then carries terms of the size of the depth spread within the pixel instead of the depth
    // itself (the values differ little along a list, and R is a running difference: SURVEY B.4).
    float dpz[SPW], v0[SPW], azS[SPW], azT[SPW], azA[SPW];
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        const int pyl = tyl * kTile + row + 4 * p;
        pfy[p] = (float)pyl;
        const bool in = px < geo.W && pyl < geo.vh;
        const size_t pix = in ? (size_t)pyl * geo.W + px : 0;
        const float Tfin = in ? final_T[pix] : 1.0f;
        dp0[p] = in ? dL_dpix[pix] : 0.0f;
        dp1[p] = in ? dL_dpix[npix + pix] : 0.0f;
        dp2[p] = in ? dL_dpix[2 * npix + pix] : 0.0f;
        const float sdp = in ? accum[pix] * dp0[p] + accum[npix + pix] * dp1[p] + accum[2 * npix + pix] * dp2[p]
                             : 0.0f;
        R[p] = sdp + Tfin * (geo.bg0 * dp0[p] + geo.bg1 * dp1[p] + geo.bg2 * dp2[p]);
        dpz[p] = 0.0f;
        if constexpr (AUX) {
            // the depth channel is a fourth colour without background; alpha = 1 - T_final, so its
            // gradient enters like a background of -dL/dalpha (both added to R below, once the
            // chunk's start is known)
            dpz[p] = in && ax.dL_ddepth ? ax.dL_ddepth[pix] : 0.0f;
            azA[p] = in && ax.dL_dalpha ? ax.dL_dalpha[pix] : 0.0f;
            azS[p] = in ? ax.accum_z[pix] : 0.0f;
            azT[p] = Tfin;
            const float atot = 1.0f - Tfin;
            v0[p] = atot > 1e-6f ? azS[p] / atot : 0.0f;
        } else {
            v0[p] = azS[p] = azT[p] = azA[p] = 0.0f;
        }
        T[p] = in ? 1.0f : -1.0f;
    }
    if (chunk > 0) {  // resume from F6's checkpoint: T, and R less dL/dpix . (colour sum so far)
        const size_t slot = ck_slot_of(geo.ck_fixed, range.x, tl, chunk);
        const float4* src = ck + slot * 256;
        // F6's live-stripe bytes: a stripe it did not write had finished (start it dead)
        const uint32_t on = *reinterpret_cast<const uint32_t*>(
            reinterpret_cast<const uint8_t*>(ck + (size_t)geo.ck_slots * 256) + 4 * slot);
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            if ((on >> (8 * p)) & 0xFFu) {  // wave-uniform
                const float4 c4 = src[64 * p + col + 16 * row];  // F6's lane of this pixel
                T[p] = c4.x;
                R[p] -= fmaf(c4.y, dp0[p], fmaf(c4.z, dp1[p], c4.w * dp2[p]));
                if constexpr (AUX) azS[p] -= ax.ckz[slot * 256 + 64 * p + col + 16 * row];
            } else {
                T[p] = -1.0f;
            }
        }
    }
    if constexpr (AUX) {
        // the depth and alpha terms of R at this chunk's start (azS: the depth sum from here on).  Both
        // products are exact zeros when the aux gradients are absent, and R is then the plain kernel's,
        // bit for bit.
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            const float Tst = chunk > 0 ? fabsf(T[p]) : 1.0f;
            const float rem = azS[p] - v0[p] * (Tst - azT[p]);  // sum over the records ahead of w (v - v0)
            R[p] = R[p] + ((rem - (v0[p] + vref) * azT[p]) * dpz[p] - azT[p] * azA[p]);
        }
    }
    // F6 wrote the stripe mask of every entry it loaded, all before its termination index tend;
    // past tend no pixel is live
    const int n_lim = n < (int)tend ? n : (int)tend;
    const FlushLane flane = flush_lane<AUX>(lane, qpark, p8f, p1, ax.pz);
    for (int base = start; base < n_lim;) {
        uint32_t live = 0;  // in stripe positions (the mask bytes' bits)
#pragma unroll
        for (int p = 0; p < SPW; ++p) live |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
        if (live == 0) break;
        // the batch: up to 64 entries with a live stripe among the next 256 (four mask bytes
        // per lane from one aligned word), in list order; the next batch starts after the last
        // one taken, or after the window
        static_assert(kB1Win == 4, "one mask word and four gids per lane");
        const uint32_t a0 = (range.x + (uint32_t)base) & ~(uint32_t)(kB1Win - 1);  // aligned window start
        const uint32_t wd = *reinterpret_cast<const uint32_t*>(mk + a0 + 4 * lane);
        // the window's gids beside its mask bytes (one 16-B load per lane; the list array is
        // followed by the rest of the binning buffer, so the window's tail past the list is
        // readable and never used): the batch's record loads then wait for no gid load
        const uint4 gw = *reinterpret_cast<const uint4*>(sorted_gid + a0 + 4 * lane);
        const uint32_t gwa[4] = {gw.x, gw.y, gw.z, gw.w};
        uint32_t vis = 0;
#pragma unroll
        for (int i = 0; i < kB1Win; ++i) {
            const int e = (int)(a0 + kB1Win * lane + i - range.x);  // list offset of byte i
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
        const uint32_t excl = incl - c;
        const uint32_t total = (uint32_t)__shfl(incl, 63, 64);
        const int cnt = total < 64u ? (int)total : 64;
        uint32_t pos = excl;
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
        // next window: after the 64th taken entry when the window held more, else past it
        base = total > 64u ? (int)lds.sidx[63] + 1 : (int)(a0 + 64 * kB1Win - range.x);
        if (cnt == 0) {
            __syncthreads();
            continue;
        }
        uint32_t jl = 0, smask = 0;
        if (lane < cnt) {
            const uint32_t g = lds.sgd[lane];
            const uint4 rr = rect[g];
            const int minx = rr.x & 0xFFFF, miny = rr.x >> 16, maxx = rr.y & 0xFFFF;
            const int y0 = miny > geo.ty0 ? miny : geo.ty0;
            jl = rr.z + (uint32_t)((ty - y0) * (maxx - minx) + (tx - minx));
            // past the capacity: an overflowing binning (the row-bucketed one keeps list
            // positions, not emission indices, below it) -- the entry is not written
            if (jl >= geo.cap) jl = 0xFFFFFFFFu;
            const float4* r = rec + 3 * (size_t)g;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            float2* const d = srec + lane * (kStagedRec / 2);
            d[0] = make_float2(r0.x, r0.y);
            d[1] = make_float2(r0.z, r0.w);
            d[2] = make_float2(r1.x, r1.z);
            d[3] = make_float2(r1.w, r2.x);
            d[4] = make_float2(r2.w, __uint_as_float(jl));
            if constexpr (AUX) svz[lane] = aux_value(ax.depth_key[g], ax.inv) - vref;
            smask = lds.smv[lane];
        }
        __syncthreads();
        uint64_t todo = __ballot(lane < cnt);
        int visited = 0, parked = 0;
        uint32_t kpack = 0;  // batch slots of the parked records, 6 bits each
        // one visited record (batch slot k): its stripes, then its moments parked / flushed;
        // true when every pixel of the tile has finished
        auto record = [&](const int k, const StagedRec sr, const float vz) -> bool {
            const float4 r0 = sr.r0, r1 = make_float4(sr.h.x, 0.0f, sr.h.y, sr.h.z), r2 = make_float4(sr.h.w, 0.0f, 0.0f, sr.L);
            const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)smask, k) & live;
            const float dx = r0.x - pfx;
            const float bdx = r0.w * dx;
            const float K = fmaf(r0.z * dx, dx, r2.w);
            // -0 is the exact identity of IEEE addition (x + -0 = x for every x, +0 included), so
            // the first stripe's adds / FMAs into these fold into plain moves / multiplies
            // without fast-math; +0 would keep them (0 + -0 = +0)
            float s0 = -0.f, sy = -0.f, syy = -0.f, g0 = -0.f, g1 = -0.f, g2 = -0.f;
            float gz = -0.f;  // aux: sum w dL/ddepth
            // lanes with a contributing pair in any stripe: the stripes' own exec masks, ORed on
            // the scalar port (a per-lane flag costs a VGPR, a move per contributing stripe and a
            // compare per record)
            uint64_t any = 0;
            // one contributing (pixel, record) pair of stripe p into the record's moments
            auto contribute = [&](const int p, const float a, const float w, const float oG, const float dy) {
                const float one_m = 1.0f - a;
                float cdp = fmaf(r1.z, dp0[p], fmaf(r1.w, dp1[p], r2.x * dp2[p]));
                if constexpr (AUX) {
                    cdp = fmaf(vz - v0[p], dpz[p], cdp);
                    gz = fmaf(w, dpz[p], gz);
                }
                R[p] = fmaf(-w, cdp, R[p]);
                const float dLda = fmaf(T[p], cdp, -R[p] * __builtin_amdgcn_rcpf(one_m));
                g0 = fmaf(w, dp0[p], g0);
                g1 = fmaf(w, dp1[p], g1);
                g2 = fmaf(w, dp2[p], g2);
                const float sv = oG * dLda;
                s0 += sv;
                const float svy = sv * dy;
                sy += svy;
                syy = fmaf(svy, dy, syy);
            };
#pragma unroll
            for (int p = 0; p < SPW; ++p) {
                if (!(m & (1u << p))) continue;  // wave-uniform
                const float dy = r0.y - pfy[p];
                const float e = fmaf(fmaf(r1.x, dy, bdx), dy, K);
                float oG;
                bool keep;
                const float a = pair_alpha_keep(e, r2.w, oG, keep);
                const float w = a * T[p];
                const float tT = T[p] - w;
                const bool ok = tT >= 0.0001f;
                // keep's two compares and ok's, each balloted on its own: the ballot of a compare is
                // the compare's SGPR mask, the ballot of their conjunction a select and a compare
                any |= __builtin_amdgcn_fcmpf(tT, 0.0001f, 3) & __builtin_amdgcn_fcmpf(e, r2.w, 5) &
                       __builtin_amdgcn_fcmpf(oG, 1.0f / 255.0f, 3);
                if (ok && keep) contribute(p, a, w, oG, dy);
                T[p] = ok ? tT : -fabsf(T[p]);
            }
            if (any) {
                // the quad shares dx: reduce the six column sums (12 DPP adds, not 18 for the
                // nine dx-weighted moments of a row-major quad), then apply dx once
                float u[AUX ? 7 : 6] = {s0, sy, syy, g0, g1, g2};
                if constexpr (AUX) u[6] = gz;
                quad_reduce(u);
                const float sx = u[0] * dx;
                float v[9] = {sx, u[1], sx * dx, u[1] * dx, u[2], u[0], u[3], u[4], u[5]};
                if ((lane & 3) == 0) {
                    float* dst = qlane + parked * kParkSlot;
                    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    dst[8] = v[8];
                    if constexpr (AUX) dst[9] = u[6];
                }
                kpack |= (uint32_t)k << (6 * parked);
                if (++parked == kPark) {
                    park_flush(flane, srec, kpack, kPark, fl);
                    parked = 0;
                    kpack = 0;
                }
            }
            if ((++visited & 7) == 0) {
                uint32_t lv = 0;
#pragma unroll
                for (int p = 0; p < SPW; ++p) lv |= __any(T[p] > 0.0f) ? (1u << p) : 0u;
                live = lv;
                if (live == 0) return true;
            }
            return false;
        };
        if constexpr (PF) {
            if (todo) {
                int ka = __builtin_ctzll(todo);
                todo &= todo - 1;
                StagedRec ra = staged(srec, ka), rb;
                float za = 0.0f, zb = 0.0f;
                if constexpr (AUX) za = svz[ka];
                while (true) {
                    const int kb = todo ? __builtin_ctzll(todo) : -1;  // wave-uniform
                    if (kb >= 0) {
                        todo &= todo - 1;
                        rb = staged(srec, kb);
                        if constexpr (AUX) zb = svz[kb];
                    }
                    if (record(ka, ra, za) || kb < 0) break;
                    ka = todo ? __builtin_ctzll(todo) : -1;
                    if (ka >= 0) {
                        todo &= todo - 1;
                        ra = staged(srec, ka);
                        if constexpr (AUX) za = svz[ka];
                    }
                    if (record(kb, rb, zb) || ka < 0) break;
                }
            }
        } else {
            while (todo) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
                float vz = 0.0f;
                if constexpr (AUX) vz = svz[k];
                if (record(k, staged(srec, k), vz)) break;
            }
        }
        if (parked) park_flush(flane, srec, kpack, parked, fl);
        __syncthreads();  // srec / qpark are rewritten by the next batch
    }
}
}  // namespace

// the aux channel comes with full images only, outside views mode
static bool aux_ok(const void* aux, const gsr_camera& cam, int ty0, int ty1, int vgy) {
    return !aux || (vgy <= 0 && ty0 == 0 && ty1 == div_up(cam.height, kTile));
}

int launch_blend_forward(const gsr_camera& cam, const float bg[3], int ty0, int ty1,
                         const uint2* ranges, const uint32_t* sorted_gid, const float4* rec,
                         float* out_color, float* final_T, float* accum, uint32_t* term, float4* ck, long long cap,
                         hipStream_t s, int vgy, int vh, uint8_t* mk, const F6Aux* aux) {
    if (!aux_ok(aux, cam, ty0, ty1, vgy)) return (int)hipErrorInvalidValue;
    const BlendGeom geo = make_geo(cam, bg, ty0, ty1, cap, vgy, vh);
    if (geo.nwg <= 0) return 0;
    auto launch = [&](auto nw, auto... ax) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((blend_forward_kernel<NW, decltype(ax)...>), dim3(geo.nwg), dim3(64 * NW), 0, s, geo, ranges,
                           sorted_gid, rec, out_color, final_T, accum, term, ck, mk, ax...);
    };
    auto pick = [&](auto... ax) {
        if (image_tiles(geo, vgy) >= kF6BandTiles)
            launch(std::integral_constant<int, kF6FullWaves>{}, ax...);
        else
            launch(std::integral_constant<int, kF6BandWaves>{}, ax...);
    };
    aux ? pick(*aux) : pick();
    return (int)hipGetLastError();
}

// B1: one one-wave block per (tile, chunk slot).  Splitting a band launch's (tile, chunk) over 2 or
// 4 waves by stripe was measured at 1M / 1080p, N = 8 (rehearsal kernel trace, mean band B1 /
// gather; profiles/r06_experiments/b1_split_1m_w8.txt): 1 part 101.8 / 24.7 us, 2 parts 101.4 /
// 50.9, 4 parts 130.0 / 115.4 -- a part repeats the record's set-up, batch loads and reduction for
// fewer stripes, and the per-chunk chain is set by that per-record work, not by the stripes.
int launch_blend_backward(const gsr_camera& cam, const float bg[3], int ty0, int ty1,
                          const uint2* ranges, const uint32_t* sorted_gid, const uint4* rect,
                          const float4* rec, const float* final_T,
                          const float* accum, const float* dL_dpix, float* partial, long long cap,
                          const uint32_t* term, const float4* ck, hipStream_t s, int vgy, int vh,
                          const uint8_t* mk, const B1Aux* aux) {
    if (!aux_ok(aux, cam, ty0, ty1, vgy)) return (int)hipErrorInvalidValue;
    const BlendGeom geo = make_geo(cam, bg, ty0, ty1, cap, vgy, vh);
    if (geo.nwg <= 0) return 0;
    const PartLayout pl(cap, aux != nullptr);
    const int blocks = 8 * (geo.nwg / 8 + 1) * kMaxChunks;
    auto launch = [&](auto pf, auto... ax) {
        hipLaunchKernelGGL((blend_backward_kernel<decltype(pf)::value, decltype(ax)...>), dim3(blocks), dim3(64), 0, s,
                           geo, ranges, sorted_gid, rect, rec, final_T, accum, dL_dpix, at<float>(partial, pl.p8),
                           at<float>(partial, pl.p1), at<uint8_t>(partial, pl.fl), term, ck, mk, ax...);
    };
    auto pick = [&](auto... ax) {
        if (image_tiles(geo, vgy) < kF6BandTiles)
            launch(std::true_type{}, ax...);  // prefetching B1
        else
            launch(std::false_type{}, ax...);
    };
    B1Aux ax = aux ? *aux : B1Aux{};
    ax.pz = at<float>(partial, pl.pz);
    aux ? pick(ax) : pick();
    return (int)hipGetLastError();
}

int launch_clear_flags(float* partial, long long cap, bool aux, hipStream_t s) {
    if (cap <= 0) return 0;
    return (int)hipMemsetAsync(at<uint8_t>(partial, PartLayout(cap, aux).fl), 0, (size_t)cap, s);
}

}  // namespace gsr

