// gsr_optim.hip -- what runs every iteration on the per-Gaussian arrays (include/gsr/gsr_train.h,
// SURVEY.md §8f rows 1-2) on gfx950, under the step guard where it writes training state.
//
//  * activate_kernel      exp / normalize / sigmoid of the raw leaves (the reference's getters,
//                         src/scene/gaussian_model.cpp:270-298), one thread per Gaussian.
//  * adam_kernel          one launch for all six parameter groups (multi-tensor): activation
//                         backward, moments, bias-corrected update; float4 per thread.
//  * adam_sparse_kernel   the same step for the rows of Gaussians with radii > 0 only: a block reads
//                         its span's radii into an LDS bitmap and fetches only the float4 pieces
//                         that overlap a visible row.
//  * densify_stats_kernel max_radii2D / grad accumulation / denom for radii > 0.
//  * mcmc_noise_kernel    the MCMC strategy's per-iteration exploration noise on the means: activations,
//                         R diag(s^2) R^T and the opacity gate fused, one thread per Gaussian on a
//                         grid-stride loop, 68 B per Gaussian.
//
// All of these are HBM-bound streams (DESIGN.md §11 gives bytes per element); none is
// GEMM-shaped, so nothing here goes near MFMA.
#include <climits>
#include <cmath>
#include <cstring>

#include "gsr/gsr_train.h"
#include "gsr_train_dev.h"

namespace gsr {
namespace {

// ---------------------------------------------------------------- activations
__global__ __launch_bounds__(256) void activate_kernel(const float* __restrict__ s_raw, const float4* __restrict__ q_raw,
                                                       const float* __restrict__ o_raw, int P, float* __restrict__ s,
                                                       float4* __restrict__ q, float* __restrict__ o) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    if (s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[3 * g + k] = expf(s_raw[3 * g + k]);
    }
    if (q) {
        const float4 r = q_raw[g];
        const float n = fmaxf(sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w), 1e-12f);
        q[g] = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
    }
    if (o) o[g] = 1.0f / (1.0f + expf(-o_raw[g]));
}

// ---------------------------------------------------------------- Adam
struct AdamArgs {
    gsr_adam_group g[GSR_ADAM_MAX_GROUPS];
    int blk_start[GSR_ADAM_MAX_GROUPS + 1];
    float step_size[GSR_ADAM_MAX_GROUPS];  // lr / (1 - beta1^step)
    float bc2_sqrt[GSR_ADAM_MAX_GROUPS];   // sqrt(1 - beta2^step)
    int ngroups;
    float b1, b2, eps, omb1, omb2;          // omb = 1 - beta (rounded once, as libtorch's alpha)
    const uint32_t* guard_k;                // skip the whole step when *guard_k > guard_cap
    uint32_t guard_cap;
};

constexpr int kAdamBlock = 256, kAdamPerBlock = 4 * kAdamBlock;

// The float4 piece at element e of a group's four arrays: one streaming load per array, or
// (cnt < 4: a group's tail) its first cnt elements with zeros past them.
__device__ __forceinline__ void adam_load(const float* P, const float* G, const float* M, const float* V, long long e,
                                          int cnt, float (&p)[4], float (&g)[4], float (&m)[4], float (&v)[4]) {
    if (cnt == 4) {
        const float4 P4 = ld4(P + e);
        const float4 G4 = ld4(G + e);
        const float4 M4 = ld4(M + e);
        const float4 V4 = ld4(V + e);
        p[0] = P4.x, p[1] = P4.y, p[2] = P4.z, p[3] = P4.w;
        g[0] = G4.x, g[1] = G4.y, g[2] = G4.z, g[3] = G4.w;
        m[0] = M4.x, m[1] = M4.y, m[2] = M4.z, m[3] = M4.w;
        v[0] = V4.x, v[1] = V4.y, v[2] = V4.z, v[3] = V4.w;
    } else {
        for (int k = 0; k < 4; ++k) {
            const bool in = k < cnt;
            p[k] = in ? P[e + k] : 0.f;
            g[k] = in ? G[e + k] : 0.f;
            m[k] = in ? M[e + k] : 0.f;
            v[k] = in ? V[e + k] : 0.f;
        }
    }
}

// Stores p, m, v of the piece's elements k with on[k].  A full piece goes as float4s, its other
// elements taking the loaded bits (p0, m0, v0) back: a select, so that a NaN computed from a
// skipped element never reaches memory.
__device__ __forceinline__ void adam_store(float* P, float* M, float* V, long long e, int cnt, const bool (&on)[4],
                                           const float (&p)[4], const float (&m)[4], const float (&v)[4],
                                           const float (&p0)[4], const float (&m0)[4], const float (&v0)[4]) {
    if (cnt == 4) {
        auto sel = [&](const float(&n)[4], const float(&o)[4]) {
            return make_float4(on[0] ? n[0] : o[0], on[1] ? n[1] : o[1], on[2] ? n[2] : o[2], on[3] ? n[3] : o[3]);
        };
        st4(P + e, sel(p, p0));
        st4(M + e, sel(m, m0));
        st4(V + e, sel(v, v0));
    } else {
        for (int k = 0; k < cnt; ++k) {
            if (!on[k]) continue;
            P[e + k] = p[k];
            M[e + k] = m[k];
            V[e + k] = v[k];
        }
    }
}

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float ss, float b2s, const AdamArgs& a) {
    m = fmaf(a.omb1, g, m * a.b1);
    v = fmaf(a.omb2 * g, g, v * a.b2);
    const float denom = sqrtf(v) / b2s + a.eps;
    p = fmaf(-ss, m / denom, p);
    return p;
}

__device__ __forceinline__ void adam_act_grad(int act, float (&p)[4], float (&g)[4]) {
    // activation backward: gradient w.r.t. the raw leaf.  Uncontracted, its two fused steps written
    // as fmaf: inlined into two kernels, it rounds alike in both (the all-visible sparse step equals
    // the dense one bit for bit) whatever the optimizer would pair up.
#pragma clang fp contract(off)
    if (act == GSR_ACT_EXP) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = g[k] * expf(p[k]);
    } else if (act == GSR_ACT_SIGMOID) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float s = 1.0f / (1.0f + expf(-p[k]));
            g[k] = g[k] * (1.0f - s) * s;
        }
    } else if (act == GSR_ACT_NORMALIZE4) {  // one row of 4 (n % 4 == 0 checked on the host)
        const float nr = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
        const float n = fmaxf(nr, 1e-12f);
        const float dot = fmaf(g[0], p[0], g[1] * p[1]) + g[2] * p[2] + g[3] * p[3];
        // d/dx of x / max(|x|, eps): g / n - (g . x) / n^2 * d|x|/dx (the clamp passes no
        // gradient when it is active)
        const float c = nr > 1e-12f ? dot / (n * n) / nr : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = fmaf(-c, p[k], g[k] / n);
    }
}

// One float4 piece per thread (coalesced across the block); the thread's four loads are issued
// before any update so that its bytes are in flight together.
__global__ __launch_bounds__(kAdamBlock) void adam_kernel(const AdamArgs a) {
    if (guard_tripped(a.guard_k, a.guard_cap)) return;
    int gi = 0;
    while (gi + 1 < a.ngroups && (int)blockIdx.x >= a.blk_start[gi + 1]) ++gi;  // wave-uniform
    const gsr_adam_group& G = a.g[gi];
    const float ss = a.step_size[gi], b2s = a.bc2_sqrt[gi];
    const long long e0 = ((long long)(blockIdx.x - a.blk_start[gi]) * kAdamBlock + threadIdx.x) * 4;
    const long long left = G.n - e0;
    const int cnt = left <= 0 ? 0 : (left < 4 ? (int)left : 4);
    float p[4], g[4], m[4], v[4];
    adam_load(G.param, G.grad, G.exp_avg, G.exp_avg_sq, e0, cnt, p, g, m, v);
    if (cnt == 0) return;
    adam_act_grad(G.act, p, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) adam_one(p[k], g[k], m[k], v[k], ss, b2s, a);
    const bool all[4] = {true, true, true, true};
    adam_store(G.param, G.exp_avg, G.exp_avg_sq, e0, cnt, all, p, m, v, p, m, v);
}

// The visibility-masked step (gsr_adam_step_sparse): rows of Gaussians with radii <= 0 keep their
// bytes and are not fetched.  A block owns one group and a span of Gaussians that starts on a
// multiple of 4 (so the span's first float is float4-aligned for every row width); the host
// sizes the span so that the block walks about kSparseIters float4 pieces per thread.
constexpr int kSparseIters = 3, kSparseSpanMax = 1024;
struct AdamSparseArgs {
    AdamArgs a;
    const int* radii;
    int P;
    int width[GSR_ADAM_MAX_GROUPS];  // floats per Gaussian (n / P)
    int span[GSR_ADAM_MAX_GROUPS];   // Gaussians per block: a multiple of 4, <= kSparseSpanMax
};

// The span's radii first (coalesced, one ballot per wave into an LDS bitmap); a span without a
// visible row ends there.  Otherwise the span's flat float4 pieces as adam_kernel walks them, a
// piece's four arrays loaded only when it overlaps a visible row.  A piece that straddles a
// visible and an invisible row (widths that are no multiple of 4) stores the loaded bits back
// for the invisible elements (adam_store's select).
__global__ __launch_bounds__(kAdamBlock) void adam_sparse_kernel(const AdamSparseArgs s) {
    const AdamArgs& a = s.a;
    if (guard_tripped(a.guard_k, a.guard_cap)) return;
    int gi = 0;
    while (gi + 1 < a.ngroups && (int)blockIdx.x >= a.blk_start[gi + 1]) ++gi;  // wave-uniform
    const gsr_adam_group& G = a.g[gi];
    const float ss = a.step_size[gi], b2s = a.bc2_sqrt[gi];
    const int width = s.width[gi], span = s.span[gi];
    const int g0 = (int)(blockIdx.x - a.blk_start[gi]) * span;
    const int len = min(span, s.P - g0);
    __shared__ unsigned long long vis[kSparseSpanMax / 64 + 1];  // + 1: the row after a full span's last
    bool mine = false;
    for (int j0 = 0; j0 < len; j0 += kAdamBlock) {  // block-uniform trip count
        const int j = j0 + (int)threadIdx.x;
        const bool on = j < len && s.radii[g0 + j] > 0;
        const unsigned long long bits = __ballot(on);
        if ((threadIdx.x & 63) == 0) vis[j >> 6] = bits;
        mine |= on;
    }
    if (!__syncthreads_or(mine)) return;
    float* const P_ = G.param + (long long)g0 * width;
    const float* const G_ = G.grad + (long long)g0 * width;
    float* const M_ = G.exp_avg + (long long)g0 * width;
    float* const V_ = G.exp_avg_sq + (long long)g0 * width;
    const int nel = len * width;  // < 2^31 (host check)
    for (int e0 = (int)threadIdx.x * 4; e0 < nel; e0 += 4 * kAdamBlock) {
        const int cnt = min(4, nel - e0);
        int row = (int)((unsigned)e0 / (unsigned)width), col = e0 - row * width;
        bool on[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            on[k] = k < cnt && ((vis[row >> 6] >> (row & 63)) & 1ull);
            any |= on[k];
            if (++col == width) col = 0, ++row;
        }
        if (!any) continue;
        float p[4], g[4], m[4], v[4];
        adam_load(P_, G_, M_, V_, e0, cnt, p, g, m, v);
        const float p0[4] = {p[0], p[1], p[2], p[3]}, m0[4] = {m[0], m[1], m[2], m[3]},
                    v0[4] = {v[0], v[1], v[2], v[3]};
        adam_act_grad(G.act, p, g);
#pragma unroll
        for (int k = 0; k < 4; ++k) adam_one(p[k], g[k], m[k], v[k], ss, b2s, a);
        adam_store(P_, M_, V_, e0, cnt, on, p, m, v, p0, m0, v0);
    }
}

// ---------------------------------------------------------------- densification statistics
__global__ __launch_bounds__(256) void densify_stats_kernel(const int* __restrict__ radii, const float* __restrict__ dm2,
                                                            int P, float* __restrict__ maxr, float* __restrict__ acc,
                                                            float* __restrict__ den, const uint32_t* guard_k,
                                                            uint32_t guard_cap) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P || guard_tripped(guard_k, guard_cap)) return;
    const int r = radii[g];
    if (r <= 0) return;
    maxr[g] = fmaxf(maxr[g], (float)r);
    const float gx = dm2[3 * g], gy = dm2[3 * g + 1];
    acc[g] += sqrtf(gx * gx + gy * gy);
    den[g] += 1.0f;
}

// ---------------------------------------------------------------- MCMC exploration noise
// gsr_mcmc_noise: xyz += Sigma (noise * gate * strength), Sigma = R diag(s^2) R^T from the RAW leaves
// (the step's activated tensors are stale after the Adam step), gate = 1 / (1 + exp(100 (o - 0.005))).
// One thread per Gaussian on a grid-stride loop; a thread's five loads are issued before any use.
// Traffic per Gaussian: xyz 12 + 12, scales 12, rotation 16 (one float4), opacity 4, noise 12 = 68 B.
constexpr int kNoiseBlock = 256, kNoiseMaxBlocks = 2048;

__global__ __launch_bounds__(kNoiseBlock) void mcmc_noise_kernel(float* __restrict__ xyz, const float* __restrict__ s_raw,
                                                                 const float4* __restrict__ q_raw,
                                                                 const float* __restrict__ o_raw,
                                                                 const float* __restrict__ noise, int P, float strength,
                                                                 const uint32_t* guard_k, uint32_t guard_cap) {
    if (guard_tripped(guard_k, guard_cap)) return;
    const long long stride = (long long)gridDim.x * kNoiseBlock;
    for (long long g = (long long)blockIdx.x * kNoiseBlock + threadIdx.x; g < P; g += stride) {
        const float4 r = q_raw[g];
        const float oraw = o_raw[g];
        float x[3], sr[3], nz[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = xyz[3 * g + k];
            sr[k] = s_raw[3 * g + k];
            nz[k] = noise[3 * g + k];
        }
        const float o = 1.0f / (1.0f + expf(-oraw));
        // exp overflows to +inf from o ~ 0.89 on: 1 / (1 + inf) = 0 is the intended gate, and a zero
        // gate ends the row here -- its xyz keeps its bits, and no inf ever meets a 0
        const float gate = 1.0f / (1.0f + expf(100.0f * (o - 0.005f)));
        if (gate == 0.0f) continue;
        const float n = fmaxf(sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w), 1e-12f);
        const float qr = r.x / n, qx = r.y / n, qy = r.z / n, qz = r.w / n;  // w first
        // general.build_rotation, row-major
        const float R[3][3] = {{1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qr * qz), 2.f * (qx * qz + qr * qy)},
                               {2.f * (qx * qy + qr * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qr * qx)},
                               {2.f * (qx * qz - qr * qy), 2.f * (qy * qz + qr * qx), 1.f - 2.f * (qx * qx + qy * qy)}};
        const float gs = gate * strength;
        const float v[3] = {nz[0] * gs, nz[1] * gs, nz[2] * gs};
        float t[3];  // diag(s^2) R^T v
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = expf(sr[k]);
            t[k] = (s * s) * (R[0][k] * v[0] + R[1][k] * v[1] + R[2][k] * v[2]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) xyz[3 * g + k] = x[k] + (R[k][0] * t[0] + R[k][1] * t[1] + R[k][2] * t[2]);
    }
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_activate(const float* scale_raw, const float* rot_raw, const float* opac_raw, int32_t P, float* scales,
                 float* rots, float* opacs, void* stream) {
    if (P < 0) return set_error(-1, "activate: negative P");
    if (P == 0) return 0;
    if ((scales && !scale_raw) || (rots && !rot_raw) || (opacs && !opac_raw)) return set_error(-1, "activate: null input");
    if (!all_aligned16({rots, rot_raw})) return set_error(-1, "activate: rotations must be 16-byte aligned");
    hipLaunchKernelGGL(activate_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, scale_raw,
                       reinterpret_cast<const float4*>(rot_raw), opac_raw, P, scales, reinterpret_cast<float4*>(rots),
                       opacs);
    return (int)hipGetLastError();
}

int gsr_adam_step(const gsr_adam_group* groups, int32_t ngroups, float beta1, float beta2, float eps, void* stream) {
    return gsr_adam_step_guarded(groups, ngroups, beta1, beta2, eps, nullptr, 0, stream);
}

// The checks and the per-group scalars the dense and the sparse step share: everything of AdamArgs
// but blk_start (1 <= ngroups <= GSR_ADAM_MAX_GROUPS).  0, or < 0 with the error text set.
static int adam_fill_args(AdamArgs& a, const gsr_adam_group* groups, int32_t ngroups, float beta1, float beta2, float eps,
                          const uint32_t* guard_k, uint32_t guard_cap) {
    if (!groups) return set_error(-1, "adam: null groups");
    std::memset(&a, 0, sizeof a);
    a.ngroups = ngroups;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    a.omb1 = (float)(1.0 - (double)beta1);
    a.omb2 = (float)(1.0 - (double)beta2);
    a.guard_k = guard_k;
    a.guard_cap = guard_cap;
    for (int i = 0; i < ngroups; ++i) {
        const gsr_adam_group& g = groups[i];
        if (g.n < 0) return set_error(-1, "adam: negative group size");
        if (g.n > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)) return set_error(-1, "adam: null tensor");
        if (g.step < 1) return set_error(-1, "adam: step must be >= 1");
        if (g.act < GSR_ACT_NONE || g.act > GSR_ACT_NORMALIZE4) return set_error(-1, "adam: bad activation");
        if (g.act == GSR_ACT_NORMALIZE4 && g.n % 4) return set_error(-1, "adam: normalize group needs rows of 4");
        if (!all_aligned16({g.param, g.grad, g.exp_avg, g.exp_avg_sq}))
            return set_error(-1, "adam: tensors must be 16-byte aligned");
        a.g[i] = g;
        // libtorch adam.cpp: bias corrections in double, scalars cast to the tensor type
        const double bc1 = 1.0 - std::pow((double)beta1, (double)g.step);
        const double bc2 = 1.0 - std::pow((double)beta2, (double)g.step);
        a.step_size[i] = (float)((double)g.lr / bc1);
        a.bc2_sqrt[i] = (float)std::sqrt(bc2);
    }
    return 0;
}

int gsr_adam_step_guarded(const gsr_adam_group* groups, int32_t ngroups, float beta1, float beta2, float eps,
                          const uint32_t* guard_k, uint32_t guard_cap, void* stream) {
    if (ngroups < 0 || ngroups > GSR_ADAM_MAX_GROUPS) return set_error(-1, "adam: 0..8 groups");
    if (ngroups == 0) return 0;
    AdamArgs a;
    if (const int rc = adam_fill_args(a, groups, ngroups, beta1, beta2, eps, guard_k, guard_cap)) return rc;
    long long blocks = 0;
    for (int i = 0; i < ngroups; ++i) {
        a.blk_start[i] = (int)blocks;
        blocks += (a.g[i].n + kAdamPerBlock - 1) / kAdamPerBlock;
        if (blocks > INT32_MAX / 2) return set_error(-1, "adam: too many elements");
    }
    a.blk_start[ngroups] = (int)blocks;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(kAdamBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int gsr_adam_step_sparse(const gsr_adam_group* groups, int32_t ngroups, const int32_t* radii, int32_t P, float beta1,
                         float beta2, float eps, const uint32_t* guard_k, uint32_t guard_cap, void* stream) {
    if (ngroups < 0 || ngroups > GSR_ADAM_MAX_GROUPS) return set_error(-1, "adam: 0..8 groups");
    if (P < 0) return set_error(-1, "adam: negative P");
    if (ngroups == 0 || P == 0) return 0;
    if (!radii) return set_error(-1, "adam: null radii");
    AdamSparseArgs s;
    std::memset(&s, 0, sizeof s);
    if (const int rc = adam_fill_args(s.a, groups, ngroups, beta1, beta2, eps, guard_k, guard_cap)) return rc;
    s.radii = radii;
    s.P = P;
    long long blocks = 0;
    for (int i = 0; i < ngroups; ++i) {
        const gsr_adam_group& g = s.a.g[i];
        s.a.blk_start[i] = (int)blocks;
        if (g.n == 0) continue;  // e.g. f_rest at SH degree 0
        if (g.n % P) return set_error(-1, "adam: group size is no multiple of P");
        const long long width = g.n / P;
        if (g.act == GSR_ACT_NORMALIZE4 && width % 4) return set_error(-1, "adam: normalize group needs rows of 4");
        if (width >= (1ll << 28)) return set_error(-1, "adam: row too wide");  // 4 rows' floats stay in int32
        // about kSparseIters float4 pieces per thread; 4 | span keeps every span float4-aligned
        long long span = (long long)kSparseIters * kAdamPerBlock / width;
        span = (span < kSparseSpanMax ? span : kSparseSpanMax) & ~3ll;
        if (span < 4) span = 4;
        s.width[i] = (int)width;
        s.span[i] = (int)span;
        blocks += (P + span - 1) / span;
    }
    if (blocks > INT32_MAX / 2) return set_error(-1, "adam: too many elements");
    s.a.blk_start[ngroups] = (int)blocks;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(adam_sparse_kernel, dim3((unsigned)blocks), dim3(kAdamBlock), 0, (hipStream_t)stream, s);
    return (int)hipGetLastError();
}

int gsr_densify_stats(const int32_t* radii, const float* dmeans2D, int32_t P, float* max_radii2D, float* grad_accum,
                      float* denom, void* stream) {
    return gsr_densify_stats_guarded(radii, dmeans2D, P, max_radii2D, grad_accum, denom, nullptr, 0, stream);
}

int gsr_densify_stats_guarded(const int32_t* radii, const float* dmeans2D, int32_t P, float* max_radii2D,
                              float* grad_accum, float* denom, const uint32_t* guard_k, uint32_t guard_cap,
                              void* stream) {
    if (P < 0) return set_error(-1, "densify_stats: negative P");
    if (P == 0) return 0;
    if (!radii || !dmeans2D || !max_radii2D || !grad_accum || !denom) return set_error(-1, "densify_stats: null tensor");
    hipLaunchKernelGGL(densify_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, radii, dmeans2D, P,
                       max_radii2D, grad_accum, denom, guard_k, guard_cap);
    return (int)hipGetLastError();
}

int gsr_mcmc_noise(float* xyz, const float* scale_raw, const float* rot_raw, const float* opac_raw, const float* noise,
                   int32_t P, float strength, const uint32_t* guard_k, uint32_t guard_cap, void* stream) {
    if (P < 0) return set_error(-1, "mcmc_noise: negative P");
    if (!(strength >= 0.0f) || std::isinf(strength)) return set_error(-1, "mcmc_noise: strength must be finite and >= 0");
    if (P == 0) return 0;
    if (!xyz || !scale_raw || !rot_raw || !opac_raw || !noise) return set_error(-1, "mcmc_noise: null pointer");
    if (!all_aligned16({rot_raw})) return set_error(-1, "mcmc_noise: rotations must be 16-byte aligned");
    for (const void* p : {(const void*)xyz, (const void*)scale_raw, (const void*)opac_raw, (const void*)noise})
        if (reinterpret_cast<uintptr_t>(p) & 3) return set_error(-1, "mcmc_noise: tensors must be 4-byte aligned");
    if (strength == 0.0f) return 0;  // a zero displacement: xyz keeps its bytes
    const long long want = ((long long)P + kNoiseBlock - 1) / kNoiseBlock;
    const int nb = (int)(want < kNoiseMaxBlocks ? want : kNoiseMaxBlocks);
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(nb), dim3(kNoiseBlock), 0, (hipStream_t)stream, xyz, scale_raw,
                       reinterpret_cast<const float4*>(rot_raw), opac_raw, noise, P, strength, guard_k, guard_cap);
    return (int)hipGetLastError();
}

}  // extern "C"
