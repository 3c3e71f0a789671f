// gsr_train.hip -- training-step kernels around the rasterizer (include/gsr/gsr_train.h,
// SURVEY.md §8f rows 1-2) on gfx950.
//
//  * activate_kernel      exp / normalize / sigmoid of the raw leaves (the reference's getters,
//                         src/scene/gaussian_model.cpp:270-298), one thread per Gaussian.
//  * ssim_forward_kernel  L1 + SSIM terms of one 64 x 16 output tile per block: the raw tile
//                         plus a 5-pixel halo is staged in LDS, blurred horizontally (5 moment
//                         maps) into LDS and vertically in registers (each pass slides the
//                         11-tap window over 4 outputs per thread); writes the three SSIM
//                         derivative maps the backward blurs, and one (sum S, sum |x - y|)
//                         partial per block (fixed-order sums, no atomics).
//  * ssim_backward_kernel the adjoint: blur of the three maps (same separable window) combined
//                         with x and y, plus the L1 sign term -> dL/dimg.
//  * depth_loss_kernel    weight * mean |(pred - target) * mask| over an H x W depth plane (pred = the
//                         blended depth, or depth / alpha) and dL/ddepth, dL/dalpha in the same pass:
//                         float4 per thread, one (sum |e|, count) partial per block, summed in
//                         double by depth_loss_finalize_kernel (fixed order, no atomics).
//  * exposure_*_kernel    the trained per-view 3 x 4 colour transform on the render (upstream's
//                         use_trained_exp) and its adjoint: 4 pixels of all three planes per thread,
//                         dL/dimg and one 12-float partial of dL/dexposure per block, summed in double
//                         by exposure_finalize_kernel (fixed order, no atomics).
//  * adam_kernel          one launch for all six parameter groups (multi-tensor): activation
//                         backward, moments, bias-corrected update; float4 per thread.
//  * adam_sparse_kernel   the same step for the rows of Gaussians with radii > 0 only: a block reads
//                         its span's radii into an LDS bitmap and fetches only the float4 pieces
//                         that overlap a visible row.
//  * densify_stats_kernel max_radii2D / grad accumulation / denom for radii > 0.
//  * mcmc_noise_kernel    the MCMC strategy's per-iteration exploration noise on the means: activations,
//                         R diag(s^2) R^T and the opacity gate fused, one thread per Gaussian on a
//                         grid-stride loop, 68 B per Gaussian.
//  * mcmc_relocate_kernel the opacity / scale a relocated Gaussian and its copies take (refinements
//                         only): the binomial sum in fp64, one thread per sampled row.
//  * compact_* + gather_rows_kernel  mask -> ascending index list (wave64 ballot counts,
//                         block-local scan) and a multi-tensor row gather (prune / clone).
//
// All of these are HBM-bound streams (DESIGN.md §11 gives bytes per element); none is
// GEMM-shaped, so nothing here goes near MFMA.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "../../include/gsr/gsr_train.h"

namespace gsr {
// defined in gsr_api.cpp: sets the thread-local error text read by gsr_last_error()
int set_error(int code, const char* msg);
}  // namespace gsr

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

// ---------------------------------------------------------------- SSIM + L1
constexpr int kWin = 11, kRad = 5;
constexpr int kTX = 64, kTY = 16;                              // output tile
constexpr int kRX = kTX + 2 * kRad, kRY = kTY + 2 * kRad;      // 74 x 26 staged tile
constexpr int kRXP = kRX + 1;                                  // LDS row pitch
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct Window {
    float w[kWin];
};

__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    // fixed-order block reduction of two values (256 threads)
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

// maps: A | B | Cm planes of C*H*W floats, scaled by g = -lambda / (C H W) (dL/dS per pixel):
//   A = g dS/dmu_x, B = g dS/dE[x^2], Cm = g dS/dE[xy]
__global__ __launch_bounds__(256) void ssim_forward_kernel(const float* __restrict__ img, const float* __restrict__ gt,
                                                           int H, int W, const Window win, float gscale,
                                                           float* __restrict__ maps, float2* __restrict__ part) {
    __shared__ float sx[kRY * kRXP], sy[kRY * kRXP];
    __shared__ float hs[5][kRY * kTX];
    __shared__ float red[8];
    const int c = blockIdx.z, x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, tid = threadIdx.x;
    const size_t plane = (size_t)H * W;
    const float* X = img + c * plane;
    const float* Y = gt + c * plane;
    for (int i = tid; i < kRY * kRX; i += 256) {
        const int r = i / kRX, cc = i - r * kRX;
        const int gy = y0 - kRad + r, gx = x0 - kRad + cc;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t o = in ? (size_t)gy * W + gx : 0;
        sx[r * kRXP + cc] = in ? X[o] : 0.0f;
        sy[r * kRXP + cc] = in ? Y[o] : 0.0f;
    }
    __syncthreads();
    // horizontal pass: a thread slides the window over 4 adjacent columns of one row (14 LDS reads
    // of x and y for 4 outputs instead of 44); each output still sums its taps in k order
    for (int i = tid; i < kRY * (kTX / 4); i += 256) {
        const int r = i / (kTX / 4), c0 = 4 * (i - r * (kTX / 4));
        float m[4][5];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[j][q] = 0.f;
#pragma unroll
        for (int t = 0; t < kWin + 3; ++t) {
            const float a = sx[r * kRXP + c0 + t], b = sy[r * kRXP + c0 + t];
            const float aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = t - j;
                if (k < 0 || k >= kWin) continue;
                const float w = win.w[k];
                m[j][0] = fmaf(w, a, m[j][0]);
                m[j][1] = fmaf(w, b, m[j][1]);
                m[j][2] = fmaf(w, aa, m[j][2]);
                m[j][3] = fmaf(w, bb, m[j][3]);
                m[j][4] = fmaf(w, ab, m[j][4]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) hs[q][r * kTX + c0 + j] = m[j][q];
    }
    __syncthreads();
    float ssum = 0.f, l1sum = 0.f;
    const size_t all = (size_t)gridDim.z * plane;
    float* A = maps;
    float* B = maps + all;
    float* Cm = maps + 2 * all;
    // vertical pass: thread (column cc, row group rg) slides over rows 4 rg .. 4 rg + 3 (14 LDS
    // reads per moment for 4 outputs instead of 44), taps summed in k order as before
    const int cc = tid & (kTX - 1), r0 = 4 * (tid >> 6);
    float mv[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) mv[j][q] = 0.f;
#pragma unroll
    for (int t = 0; t < kWin + 3; ++t) {
        float h[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) h[q] = hs[q][(r0 + t) * kTX + cc];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = t - j;
            if (k < 0 || k >= kWin) continue;
            const float w = win.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) mv[j][q] = fmaf(w, h[q], mv[j][q]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + j;
        const int gx = x0 + cc, gy = y0 + r;
        const float* m = mv[j];
        if (gx >= W || gy >= H) continue;
        const float mu1 = m[0], mu2 = m[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        const float N1 = 2.0f * mu12 + kC1, N2 = 2.0f * s12 + kC2;
        const float D1 = mu1_sq + mu2_sq + kC1, D2 = s1 + s2 + kC2;
        const float den = D1 * D2;
        const float S = (N1 * N2) / den;
        const float iD1 = 1.0f / D1, iD2 = 1.0f / D2;
        const float dmu = 2.0f * mu2 * (N2 - N1) / den - 2.0f * mu1 * S * (iD1 - iD2);
        const float dxx = -S * iD2;
        const float dxy = 2.0f * N1 / den;
        const size_t o = c * plane + (size_t)gy * W + gx;
        A[o] = gscale * dmu;
        B[o] = gscale * dxx;
        Cm[o] = gscale * dxy;
        ssum += S;
        l1sum += fabsf(sx[(r + kRad) * kRXP + cc + kRad] - sy[(r + kRad) * kRXP + cc + kRad]);
    }
    block_sum2(ssum, l1sum, red);
    if (tid == 0) part[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_float2(ssum, l1sum);
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const float2* __restrict__ part, int nparts, double inv_n,
                                                            float lambda, float* __restrict__ stats) {
    __shared__ double rs[256], rl[256];
    double s = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float2 p = part[i];
        s += (double)p.x;
        l += (double)p.y;
    }
    rs[threadIdx.x] = s;
    rl[threadIdx.x] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            rs[threadIdx.x] += rs[threadIdx.x + o];
            rl[threadIdx.x] += rl[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float ssim = (float)(rs[0] * inv_n), l1 = (float)(rl[0] * inv_n);
        stats[0] = (1.0f - lambda) * l1 + lambda * (1.0f - ssim);
        stats[1] = l1;
        stats[2] = ssim;
    }
}

__global__ __launch_bounds__(256) void ssim_backward_kernel(const float* __restrict__ img, const float* __restrict__ gt,
                                                            int H, int W, const Window win, float l1scale,
                                                            const float* __restrict__ maps, float* __restrict__ dimg) {
    __shared__ float sm[3][kRY * kRXP];
    __shared__ float hs[3][kRY * kTX];
    const int c = blockIdx.z, x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, tid = threadIdx.x;
    const size_t plane = (size_t)H * W, all = (size_t)gridDim.z * plane;
    for (int i = tid; i < kRY * kRX; i += 256) {
        const int r = i / kRX, cc = i - r * kRX;
        const int gy = y0 - kRad + r, gx = x0 - kRad + cc;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t o = c * plane + (in ? (size_t)gy * W + gx : 0);
#pragma unroll
        for (int q = 0; q < 3; ++q) sm[q][r * kRXP + cc] = in ? maps[q * all + o] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kRY * (kTX / 4); i += 256) {  // horizontal, 4 columns per thread
        const int r = i / (kTX / 4), c0 = 4 * (i - r * (kTX / 4));
        float m[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) m[j][q] = 0.f;
#pragma unroll
        for (int t = 0; t < kWin + 3; ++t) {
            float v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = sm[q][r * kRXP + c0 + t];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = t - j;
                if (k < 0 || k >= kWin) continue;
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 3; ++q) m[j][q] = fmaf(w, v[q], m[j][q]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) hs[q][r * kTX + c0 + j] = m[j][q];
    }
    __syncthreads();
    const int cc = tid & (kTX - 1), r0 = 4 * (tid >> 6);  // vertical, 4 rows per thread
    float mv[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) mv[j][q] = 0.f;
#pragma unroll
    for (int t = 0; t < kWin + 3; ++t) {
        float h[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) h[q] = hs[q][(r0 + t) * kTX + cc];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = t - j;
            if (k < 0 || k >= kWin) continue;
            const float w = win.w[k];
#pragma unroll
            for (int q = 0; q < 3; ++q) mv[j][q] = fmaf(w, h[q], mv[j][q]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gx = x0 + cc, gy = y0 + r0 + j;
        if (gx >= W || gy >= H) continue;
        const size_t o = c * plane + (size_t)gy * W + gx;
        const float x = img[o], y = gt[o];
        const float d = x - y;
        const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        dimg[o] = fmaf(l1scale, sgn, mv[j][0] + 2.0f * x * mv[j][1] + y * mv[j][2]);
    }
}

// ---------------------------------------------------------------- depth L1
// weight * mean |(pred - target) * mask| and its gradient in one pass (the gradient of an L1 mean
// does not depend on the sum): a block takes chunks of 256 x 4 consecutive pixels, chunk c of
// block b being b + c * gridDim.x, and the grid depends on H * W alone, so the partial sums and
// their order -- hence the bits -- are a function of the inputs only.
constexpr int kDepthBlock = 256, kDepthChunk = 4 * kDepthBlock, kDepthMaxBlocks = 2048;

struct DepthLossArgs {
    const float* depth;
    const float* alpha;   // NORMALIZED only
    const float* target;
    const float* mask;    // nullable: 1
    float* d_depth;
    float* d_alpha;       // NORMALIZED only
    long long n;
    float gscale;         // weight / n
    float alpha_min;
    int mode;
};

__host__ __device__ inline long long depth_loss_chunks(long long n) { return (n + kDepthChunk - 1) / kDepthChunk; }
inline int depth_loss_blocks(long long n) {
    const long long c = depth_loss_chunks(n);
    return (int)(c < kDepthMaxBlocks ? (c > 0 ? c : 1) : kDepthMaxBlocks);
}

// V4: a full group of 4 pixels on 16-byte-aligned planes (one float4 access per plane); otherwise
// `cnt` <= 4 pixels with scalar accesses.
template <bool V4>
__device__ __forceinline__ void depth_load4(const float* p, long long e0, int cnt, float (&v)[4]) {
    if (V4) {
        const float4 q = *reinterpret_cast<const float4*>(p + e0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[e0 + k] : 0.f;
    }
}

template <bool V4>
__device__ __forceinline__ void depth_store4(float* p, long long e0, int cnt, const float (&v)[4]) {
    if (V4) {
        *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) p[e0 + k] = v[k];
    }
}

// the pixels e0 .. e0 + cnt - 1 of one thread: gradients out, (sum |e|, count) into the thread's sums
template <bool V4>
__device__ __forceinline__ void depth_loss_group(const DepthLossArgs& a, long long e0, int cnt, float& asum,
                                                 float& cnt_sum) {
#pragma clang fp contract(off)  // both instantiations round alike: float4 and scalar paths, same bits
    const bool norm = a.mode == GSR_DEPTH_NORMALIZED;
    float d[4], t[4], m[4], al[4] = {0.f, 0.f, 0.f, 0.f}, gd[4], ga[4];
    depth_load4<V4>(a.depth, e0, cnt, d);
    depth_load4<V4>(a.target, e0, cnt, t);
    if (a.mask) {
        depth_load4<V4>(a.mask, e0, cnt, m);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = k < cnt ? 1.f : 0.f;
    }
    if (norm) depth_load4<V4>(a.alpha, e0, cnt, al);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // a pixel below alpha_min (alpha_min > 0, so alpha = 0 never divides) contributes nothing
        const bool ok = !norm || al[k] >= a.alpha_min;
        const float inv = norm ? (ok ? 1.0f / al[k] : 0.f) : 1.0f;
        const float mk = ok ? m[k] : 0.f;
        const float pred = norm ? d[k] * inv : d[k];
        const float e = ok ? (pred - t[k]) * mk : 0.f;
        const float sgn = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
        const float gp = a.gscale * mk * sgn;  // dL/dpred
        gd[k] = gp * inv;
        ga[k] = ok ? -gp * d[k] * inv * inv : 0.f;
        asum += fabsf(e);
        cnt_sum += mk != 0.f ? 1.f : 0.f;
    }
    depth_store4<V4>(a.d_depth, e0, cnt, gd);
    if (norm) depth_store4<V4>(a.d_alpha, e0, cnt, ga);
}

// VEC: every plane is 16-byte aligned, so the full groups of 4 move as float4; otherwise (and for
// the image's last, partial group) the same thread moves the same pixels with scalar accesses, so
// both paths sum alike.
template <bool VEC>
__global__ __launch_bounds__(kDepthBlock) void depth_loss_kernel(const DepthLossArgs a, float2* __restrict__ part) {
    __shared__ float red[8];
    const long long chunks = depth_loss_chunks(a.n);
    float asum = 0.f, cnt_sum = 0.f;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long e0 = c * kDepthChunk + 4 * (long long)threadIdx.x;
        const long long left = a.n - e0;
        if (left <= 0) continue;
        if (VEC && left >= 4)
            depth_loss_group<true>(a, e0, 4, asum, cnt_sum);
        else
            depth_loss_group<false>(a, e0, left < 4 ? (int)left : 4, asum, cnt_sum);
    }
    block_sum2(asum, cnt_sum, red);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(asum, cnt_sum);
}

// one block: the partials in double, in index order per thread and a fixed tree across threads
__global__ __launch_bounds__(256) void depth_loss_finalize_kernel(const float2* __restrict__ part, int nparts,
                                                                  double inv_n, float weight,
                                                                  float* __restrict__ stats) {
    __shared__ double rs[256], rc[256];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float2 p = part[i];
        s += (double)p.x;
        c += (double)p.y;
    }
    rs[threadIdx.x] = s;
    rc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            rs[threadIdx.x] += rs[threadIdx.x + o];
            rc[threadIdx.x] += rc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(rs[0] * inv_n);
        stats[0] = weight * l1;
        stats[1] = l1;
        stats[2] = (float)rc[0];
    }
}

// ---------------------------------------------------------------- per-view exposure
// out = clamp?(x E[:3,:3] + E[:3,3]) over a channel-major 3 x H x W image (x a row vector per pixel,
// so the 3 x 3 part is indexed E[i][j]: input channel i, output channel j), and its adjoint.  The
// geometry is the depth loss's: a block takes chunks of 256 x 4 consecutive pixels, chunk c of
// block b being b + c * gridDim.x, on a grid that depends on H * W alone.
constexpr int kExpBlock = kDepthBlock, kExpChunk = kDepthChunk, kExpWaves = kExpBlock / 64;

// E is the row-major 3 x 4 matrix: the one expression of y_j every path evaluates (forward, and
// the backward's clamp mask), uncontracted, so that they round alike
__device__ __forceinline__ float exposure_y(const float (&E)[12], int j, float x0, float x1, float x2) {
#pragma clang fp contract(off)
    return ((E[j] * x0 + E[4 + j] * x1) + E[8 + j] * x2) + E[4 * j + 3];
}

__device__ __forceinline__ void exposure_load_matrix(const float* __restrict__ exposure, float (&E)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) E[k] = exposure[k];
}

template <bool V4>
__device__ __forceinline__ void exposure_forward_group(const float* img, float* out, const float (&E)[12],
                                                       long long n, long long e0, int cnt, bool clamp) {
    float x[3][4], y[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) depth_load4<V4>(img + i * n, e0, cnt, x[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = exposure_y(E, j, x[0][k], x[1][k], x[2][k]);
            y[k] = clamp ? fminf(fmaxf(v, 0.f), 1.f) : v;
        }
        depth_store4<V4>(out + j * n, e0, cnt, y);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kExpBlock) void exposure_forward_kernel(const float* __restrict__ img,
                                                                     const float* __restrict__ exposure, long long n,
                                                                     int clamp, float* __restrict__ out) {
    float E[12];
    exposure_load_matrix(exposure, E);
    const long long chunks = depth_loss_chunks(n);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long e0 = c * kExpChunk + 4 * (long long)threadIdx.x;
        const long long left = n - e0;
        if (left <= 0) continue;
        if (VEC && left >= 4)
            exposure_forward_group<true>(img, out, E, n, e0, 4, clamp != 0);
        else
            exposure_forward_group<false>(img, out, E, n, e0, left < 4 ? (int)left : 4, clamp != 0);
    }
}

// the pixels e0 .. e0 + cnt - 1 of one thread: dL/dimg out, the 12 sums (acc[3 i + j] = sum x_i g_j,
// acc[9 + j] = sum g_j) into the thread's accumulators.  A lane past cnt loads x = g = 0.
template <bool V4>
__device__ __forceinline__ void exposure_backward_group(const float* img, const float* dout, float* dimg,
                                                        const float (&E)[12], long long n, long long e0, int cnt,
                                                        bool clamp, float (&acc)[12]) {
#pragma clang fp contract(off)  // both instantiations round alike: float4 and scalar paths, same bits
    float x[3][4], g[3][4], d[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        depth_load4<V4>(img + i * n, e0, cnt, x[i]);
        depth_load4<V4>(dout + i * n, e0, cnt, g[i]);
    }
    if (clamp) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = exposure_y(E, j, x[0][k], x[1][k], x[2][k]);
                if (v < 0.f || v > 1.f) g[j][k] = 0.f;  // inclusive bounds, as torch.clamp's backward
            }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = (E[4 * i] * g[0][k] + E[4 * i + 1] * g[1][k]) + E[4 * i + 2] * g[2][k];
        depth_store4<V4>(dimg + i * n, e0, cnt, d);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * i + j] += x[i][k] * g[j][k];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[9 + j] += g[j][k];
    }
}

// one 12-float partial per block (3 float4 stores), reduced wave-then-block in a fixed order
template <bool VEC>
__global__ __launch_bounds__(kExpBlock) void exposure_backward_kernel(const float* __restrict__ img,
                                                                      const float* __restrict__ exposure,
                                                                      const float* __restrict__ dout, long long n,
                                                                      int clamp, float* __restrict__ dimg,
                                                                      float4* __restrict__ part) {
    __shared__ float red[kExpWaves][12];
    float E[12], acc[12];
    exposure_load_matrix(exposure, E);
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    const long long chunks = depth_loss_chunks(n);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long e0 = c * kExpChunk + 4 * (long long)threadIdx.x;
        const long long left = n - e0;
        if (left <= 0) continue;
        if (VEC && left >= 4)
            exposure_backward_group<true>(img, dout, dimg, E, n, e0, 4, clamp != 0, acc);
        else
            exposure_backward_group<false>(img, dout, dimg, E, n, e0, left < 4 ? (int)left : 4, clamp != 0, acc);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * threadIdx.x + k;
            v[k] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
        }
        part[3 * (long long)blockIdx.x + threadIdx.x] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// one block: the partials in double, in index order per thread and a fixed tree across threads;
// written (not accumulated) into the 3 x 4 layout of the parameter
__global__ __launch_bounds__(256) void exposure_finalize_kernel(const float* __restrict__ part, int nparts,
                                                                float* __restrict__ dexposure) {
    __shared__ double r[12][256];
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] += (double)part[12 * (long long)i + k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) r[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < 12; ++k) r[k][threadIdx.x] += r[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;  // k < 9: sum x_i g_j at [i][j]; k = 9 + j: sum g_j at [j][3]
        dexposure[k < 9 ? 4 * (k / 3) + k % 3 : 4 * (k - 9) + 3] = (float)r[k][0];
    }
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
constexpr int kAdamBlock = 256, kAdamVec = 1, kAdamPerBlock = 4 * kAdamVec * kAdamBlock;
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float* p, float4 v) {
    const f32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
}

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float ss, float b2s, const AdamArgs& a) {
    m = fmaf(a.omb1, g, m * a.b1);
    v = fmaf(a.omb2 * g, g, v * a.b2);
    const float denom = sqrtf(v) / b2s + a.eps;
    p = fmaf(-ss, m / denom, p);
    return p;
}

__device__ __forceinline__ void adam_act_grad(int act, float (&p)[4], float (&g)[4]) {
    // activation backward: gradient w.r.t. the raw leaf
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
        const float dot = g[0] * p[0] + g[1] * p[1] + g[2] * p[2] + g[3] * p[3];
        // d/dx of x / max(|x|, eps): g / n - (g . x) / n^2 * d|x|/dx (the clamp passes no
        // gradient when it is active)
        const float c = nr > 1e-12f ? dot / (n * n) / nr : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = g[k] / n - c * p[k];
    }
}

// kAdamVec float4 columns per thread (column u of a block is coalesced); all loads of the
// thread are issued before any update so that its bytes are in flight together.
__global__ __launch_bounds__(kAdamBlock) void adam_kernel(const AdamArgs a) {
    if (guard_tripped(a.guard_k, a.guard_cap)) return;
    int gi = 0;
    while (gi + 1 < a.ngroups && (int)blockIdx.x >= a.blk_start[gi + 1]) ++gi;  // wave-uniform
    const gsr_adam_group& G = a.g[gi];
    const float ss = a.step_size[gi], b2s = a.bc2_sqrt[gi];
    float p[kAdamVec][4], g[kAdamVec][4], m[kAdamVec][4], v[kAdamVec][4];
    long long e0[kAdamVec];
    int cnt[kAdamVec];
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
        e0[u] = (((long long)(blockIdx.x - a.blk_start[gi]) * kAdamVec + u) * kAdamBlock + threadIdx.x) * 4;
        const long long left = G.n - e0[u];
        cnt[u] = left <= 0 ? 0 : (left < 4 ? (int)left : 4);
        if (cnt[u] == 4) {
            const float4 P4 = ld4(G.param + e0[u]);
            const float4 G4 = ld4(G.grad + e0[u]);
            const float4 M4 = ld4(G.exp_avg + e0[u]);
            const float4 V4 = ld4(G.exp_avg_sq + e0[u]);
            p[u][0] = P4.x, p[u][1] = P4.y, p[u][2] = P4.z, p[u][3] = P4.w;
            g[u][0] = G4.x, g[u][1] = G4.y, g[u][2] = G4.z, g[u][3] = G4.w;
            m[u][0] = M4.x, m[u][1] = M4.y, m[u][2] = M4.z, m[u][3] = M4.w;
            v[u][0] = V4.x, v[u][1] = V4.y, v[u][2] = V4.z, v[u][3] = V4.w;
        } else {
            for (int k = 0; k < 4; ++k) {
                const bool in = k < cnt[u];
                p[u][k] = in ? G.param[e0[u] + k] : 0.f;
                g[u][k] = in ? G.grad[e0[u] + k] : 0.f;
                m[u][k] = in ? G.exp_avg[e0[u] + k] : 0.f;
                v[u][k] = in ? G.exp_avg_sq[e0[u] + k] : 0.f;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kAdamVec; ++u) {
        if (cnt[u] == 0) continue;
        adam_act_grad(G.act, p[u], g[u]);
#pragma unroll
        for (int k = 0; k < 4; ++k) adam_one(p[u][k], g[u][k], m[u][k], v[u][k], ss, b2s, a);
        if (cnt[u] == 4) {
            st4(G.param + e0[u], make_float4(p[u][0], p[u][1], p[u][2], p[u][3]));
            st4(G.exp_avg + e0[u], make_float4(m[u][0], m[u][1], m[u][2], m[u][3]));
            st4(G.exp_avg_sq + e0[u], make_float4(v[u][0], v[u][1], v[u][2], v[u][3]));
        } else {
            for (int k = 0; k < cnt[u]; ++k) {
                G.param[e0[u] + k] = p[u][k];
                G.exp_avg[e0[u] + k] = m[u][k];
                G.exp_avg_sq[e0[u] + k] = v[u][k];
            }
        }
    }
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
// for the invisible elements: a select, so that a NaN computed from an invisible row's gradient
// never reaches memory.
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
        if (cnt == 4) {
            const float4 P4 = ld4(P_ + e0);
            const float4 G4 = ld4(G_ + e0);
            const float4 M4 = ld4(M_ + e0);
            const float4 V4 = ld4(V_ + e0);
            p[0] = P4.x, p[1] = P4.y, p[2] = P4.z, p[3] = P4.w;
            g[0] = G4.x, g[1] = G4.y, g[2] = G4.z, g[3] = G4.w;
            m[0] = M4.x, m[1] = M4.y, m[2] = M4.z, m[3] = M4.w;
            v[0] = V4.x, v[1] = V4.y, v[2] = V4.z, v[3] = V4.w;
        } else {
            for (int k = 0; k < 4; ++k) {
                const bool in = k < cnt;
                p[k] = in ? P_[e0 + k] : 0.f;
                g[k] = in ? G_[e0 + k] : 0.f;
                m[k] = in ? M_[e0 + k] : 0.f;
                v[k] = in ? V_[e0 + k] : 0.f;
            }
        }
        const float p0[4] = {p[0], p[1], p[2], p[3]}, m0[4] = {m[0], m[1], m[2], m[3]},
                    v0[4] = {v[0], v[1], v[2], v[3]};
        adam_act_grad(G.act, p, g);
#pragma unroll
        for (int k = 0; k < 4; ++k) adam_one(p[k], g[k], m[k], v[k], ss, b2s, a);
        if (cnt == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                p[k] = on[k] ? p[k] : p0[k];
                m[k] = on[k] ? m[k] : m0[k];
                v[k] = on[k] ? v[k] : v0[k];
            }
            st4(P_ + e0, make_float4(p[0], p[1], p[2], p[3]));
            st4(M_ + e0, make_float4(m[0], m[1], m[2], m[3]));
            st4(V_ + e0, make_float4(v[0], v[1], v[2], v[3]));
        } else {
            for (int k = 0; k < cnt; ++k) {
                if (!on[k]) continue;
                P_[e0 + k] = p[k];
                M_[e0 + k] = m[k];
                V_[e0 + k] = v[k];
            }
        }
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

// ---------------------------------------------------------------- MCMC densification
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

// gsr_mcmc_relocate.  Binomials C(N, j), N, j <= GSR_MCMC_MAX_RATIO, by Pascal's rule at compile time:
// every entry is below 2^53 (C(51, 25) ~ 2.5e14), so the doubles are exact.
struct BinomTable {
    double c[GSR_MCMC_MAX_RATIO + 1][GSR_MCMC_MAX_RATIO + 1];
};
constexpr BinomTable make_binom_table() {
    BinomTable t{};
    for (int n = 0; n <= GSR_MCMC_MAX_RATIO; ++n) {
        t.c[n][0] = 1.0;
        for (int j = 1; j <= n; ++j) t.c[n][j] = t.c[n - 1][j - 1] + (j <= n - 1 ? t.c[n - 1][j] : 0.0);
    }
    return t;
}
__constant__ const BinomTable kBinom = make_binom_table();

// With N = the clamped ratio and x = 1 - (1 - o)^(1/N):
//   D = sum_{k=0..N-1} C(N, k+1) (-1)^k x^(k+1) / sqrt(k+1)
// (upstream's double sum over i = 1..N collapsed by the hockey-stick identity), new_scale = (o / D) scale,
// new_opacity = x clamped to [min_opacity, 1 - 2^-24].  The alternating sum loses 1.1e-3 relative in
// fp32 at o = 1 - 2^-24, N = 51; in fp64 it is good to 2e-12, so x, D and o / D are
// doubles and each output is rounded to fp32 once.  A row with o <= 0 (nothing to share: x = D = 0)
// keeps its scale and takes min_opacity.
__global__ __launch_bounds__(256) void mcmc_relocate_kernel(const float* __restrict__ opac, const float* __restrict__ scales,
                                                            const int* __restrict__ ratios, int n, float min_opacity,
                                                            float* __restrict__ new_opac, float* __restrict__ new_scales) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int N = min(max(ratios[i], 1), GSR_MCMC_MAX_RATIO);
    const double o = (double)opac[i];
    double x = 0.0, coef = 1.0;
    if (o > 0.0) {
        x = -expm1(log1p(-o) / (double)N);  // 1 - (1 - o)^(1/N) without the cancellation at small o
        double D = 0.0, xp = 1.0;
        for (int k = 0; k < N; ++k) {
            xp *= x;
            const double term = kBinom.c[N][k + 1] * xp / sqrt((double)(k + 1));
            D += (k & 1) ? -term : term;
        }
        coef = o / D;
    }
    const double hi = 1.0 - 5.9604644775390625e-8;  // 1 - 2^-24, the largest float below 1
    new_opac[i] = (float)fmin(fmax(x, (double)min_opacity), hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) new_scales[3 * (long long)i + k] = (float)(coef * (double)scales[3 * (long long)i + k]);
}

// ---------------------------------------------------------------- compaction
constexpr int kCmpBlock = 256, kCmpPer = 4 * kCmpBlock;

__device__ __forceinline__ int thread_flags(const uint8_t* mask, int n, int base, bool f[4]) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = base + k < n && mask[base + k] != 0;
        c += f[k] ? 1 : 0;
    }
    return c;
}

__global__ __launch_bounds__(kCmpBlock) void compact_count_kernel(const uint8_t* __restrict__ mask, int n,
                                                                  int* __restrict__ counts) {
    __shared__ int red[4];
    bool f[4];
    int c = thread_flags(mask, n, (blockIdx.x * kCmpBlock + threadIdx.x) * 4, f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of the block counts in one block (chunks of 1024), total -> *total
__global__ __launch_bounds__(1024) void compact_scan_kernel(int* __restrict__ counts, int nb, int* __restrict__ total) {
    __shared__ int s[1024];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const int v = i < nb ? counts[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) counts[i] = carry + s[threadIdx.x] - v;
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kCmpBlock) void compact_scatter_kernel(const uint8_t* __restrict__ mask, int n,
                                                                    const int* __restrict__ offs,
                                                                    int* __restrict__ idx) {
    __shared__ int wsum[4];
    bool f[4];
    const int base = (blockIdx.x * kCmpBlock + threadIdx.x) * 4;
    const int c = thread_flags(mask, n, base, f);
    // inclusive wave prefix of c (Hillis-Steele over 64 lanes)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o);
        if (lane >= o) x += t;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int before = offs[blockIdx.x] + x - c;
    for (int w = 0; w < wv; ++w) before += wsum[w];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (f[k]) idx[before++] = base + k;
}

// ---------------------------------------------------------------- multi-tensor row gather
struct GatherArgs {
    gsr_row_copy c[GSR_GATHER_MAX];
};

__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgs a, const int* __restrict__ idx, int n_out) {
    const gsr_row_copy& C = a.c[blockIdx.y];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tot = (long long)n_out * C.width;
    if (e >= tot) return;
    const int row = (int)(e / C.width), col = (int)(e - (long long)row * C.width);
    C.dst[e] = C.src[(long long)idx[row] * C.width + col];
}

Window ssim_window() {
    // torch: gauss = Tensor([exp(-(x - 5)^2 / (2 sigma^2)) for x in range(11)]) (double exp,
    // stored f32), then gauss / gauss.sum() in f32
    Window w;
    float g[kWin], sum = 0.0f;
    for (int x = 0; x < kWin; ++x) g[x] = (float)std::exp(-(double)((x - kRad) * (x - kRad)) / (2.0 * 1.5 * 1.5));
    for (int x = 0; x < kWin; ++x) sum += g[x];
    for (int x = 0; x < kWin; ++x) w.w[x] = g[x] / sum;
    return w;
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

int check_image(const float* img, const float* gt, int C, int H, int W) {
    if (!img || !gt) return set_error(-1, "loss: null image");
    if (C <= 0 || H <= 0 || W <= 0) return set_error(-1, "loss: bad image shape");
    return 0;
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
    if ((rots && (reinterpret_cast<uintptr_t>(rots) & 15)) || (rot_raw && (reinterpret_cast<uintptr_t>(rot_raw) & 15)))
        return set_error(-1, "activate: rotations must be 16-byte aligned");
    hipLaunchKernelGGL(activate_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, scale_raw,
                       reinterpret_cast<const float4*>(rot_raw), opac_raw, P, scales, reinterpret_cast<float4*>(rots),
                       opacs);
    return (int)hipGetLastError();
}

size_t gsr_loss_scratch_bytes(int32_t C, int32_t H, int32_t W) {
    const size_t n = (size_t)(C > 0 ? C : 0) * (H > 0 ? H : 0) * (W > 0 ? W : 0);
    const size_t nb = (size_t)((W + kTX - 1) / kTX) * ((H + kTY - 1) / kTY) * (C > 0 ? C : 0);
    return align256(3 * n * sizeof(float)) + align256(nb * sizeof(float2));
}

int gsr_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                     void* maps, float* stats, void* stream) {
    if (int e = check_image(img, gt, C, H, W)) return e;
    if (!maps || !stats) return set_error(-1, "loss: null scratch / stats");
    const dim3 grid((W + kTX - 1) / kTX, (H + kTY - 1) / kTY, C);
    const size_t n = (size_t)C * H * W;
    float* m = static_cast<float*>(maps);
    float2* part = reinterpret_cast<float2*>(static_cast<char*>(maps) + align256(3 * n * sizeof(float)));
    const float gscale = (float)(-(double)lambda_dssim / (double)n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_forward_kernel, grid, dim3(256), 0, s, img, gt, H, W, ssim_window(), gscale, m, part);
    const int nparts = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, part, nparts, 1.0 / (double)n, lambda_dssim,
                       stats);
    return (int)hipGetLastError();
}

int gsr_loss_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                      const void* maps, float* dL_dimg, void* stream) {
    if (int e = check_image(img, gt, C, H, W)) return e;
    if (!maps || !dL_dimg) return set_error(-1, "loss: null scratch / output");
    const dim3 grid((W + kTX - 1) / kTX, (H + kTY - 1) / kTY, C);
    const size_t n = (size_t)C * H * W;
    const float l1scale = (float)((1.0 - (double)lambda_dssim) / (double)n);
    hipLaunchKernelGGL(ssim_backward_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, gt, H, W, ssim_window(),
                       l1scale, static_cast<const float*>(maps), dL_dimg);
    return (int)hipGetLastError();
}

size_t gsr_depth_loss_scratch_bytes(int32_t H, int32_t W) {
    const long long n = (long long)(H > 0 ? H : 0) * (W > 0 ? W : 0);
    return align256((size_t)depth_loss_blocks(n) * sizeof(float2));
}

int gsr_depth_loss(const float* depth, const float* alpha, const float* target, const float* mask, int32_t H,
                   int32_t W, float weight, int32_t mode, float alpha_min, void* scratch, float* stats,
                   float* dL_ddepth, float* dL_dalpha, void* stream) {
    if (H <= 0 || W <= 0) return set_error(-1, "depth loss: bad image shape");
    if (!depth || !target || !scratch || !stats || !dL_ddepth) return set_error(-1, "depth loss: null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return set_error(-1, "depth loss: scratch must be 8-byte aligned");
    if (mode != GSR_DEPTH_RAW && mode != GSR_DEPTH_NORMALIZED) return set_error(-1, "depth loss: unknown mode");
    const bool norm = mode == GSR_DEPTH_NORMALIZED;
    if (norm && (!alpha || !dL_dalpha)) return set_error(-1, "depth loss: normalized mode needs alpha and dL_dalpha");
    if (norm && !(alpha_min > 0.0f)) return set_error(-1, "depth loss: alpha_min must be > 0");
    if (!(weight >= 0.0f) || std::isinf(weight)) return set_error(-1, "depth loss: weight must be finite and >= 0");
    DepthLossArgs a;
    a.depth = depth;
    a.alpha = norm ? alpha : nullptr;
    a.target = target;
    a.mask = mask;
    a.d_depth = dL_ddepth;
    a.d_alpha = norm ? dL_dalpha : nullptr;
    a.n = (long long)H * W;
    a.gscale = (float)((double)weight / (double)a.n);
    a.alpha_min = alpha_min;
    a.mode = mode;
    bool vec = true;  // the ABI takes any 4-byte-aligned plane; float4 accesses need all of them at 16
    for (const void* p : {(const void*)a.depth, (const void*)a.alpha, (const void*)a.target, (const void*)a.mask,
                          (const void*)a.d_depth, (const void*)a.d_alpha})
        if (reinterpret_cast<uintptr_t>(p) & 15) vec = false;
    const int nb = depth_loss_blocks(a.n);
    float2* part = static_cast<float2*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(depth_loss_kernel<true>, dim3(nb), dim3(kDepthBlock), 0, s, a, part);
    else
        hipLaunchKernelGGL(depth_loss_kernel<false>, dim3(nb), dim3(kDepthBlock), 0, s, a, part);
    hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3(1), dim3(256), 0, s, part, nb, 1.0 / (double)a.n, weight, stats);
    return (int)hipGetLastError();
}

size_t gsr_exposure_scratch_bytes(int32_t H, int32_t W) {
    const long long n = (long long)(H > 0 ? H : 0) * (W > 0 ? W : 0);
    return align256((size_t)depth_loss_blocks(n) * 12 * sizeof(float));
}

// the checks both exposure passes share; 0, or < 0 with the error text set
static int exposure_check(int32_t H, int32_t W, uint32_t flags, bool any_null) {
    if (H <= 0 || W <= 0) return set_error(-1, "exposure: bad image shape");
    if (any_null) return set_error(-1, "exposure: null pointer");
    if (flags & ~(uint32_t)GSR_EXPOSURE_CLAMP) return set_error(-1, "exposure: unknown flag bits");
    return 0;
}

// float4 accesses need every plane at 16 bytes: an aligned base and a plane of a multiple of 4 pixels
static bool exposure_vec(long long n, std::initializer_list<const void*> images) {
    bool vec = n % 4 == 0;
    for (const void* p : images)
        if (reinterpret_cast<uintptr_t>(p) & 15) vec = false;
    return vec;
}

int gsr_exposure_forward(const float* img, const float* exposure, int32_t H, int32_t W, uint32_t flags, float* out,
                         void* stream) {
    if (int e = exposure_check(H, W, flags, !img || !exposure || !out)) return e;
    const long long n = (long long)H * W;
    const int nb = depth_loss_blocks(n), clamp = (flags & GSR_EXPOSURE_CLAMP) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    if (exposure_vec(n, {img, out}))
        hipLaunchKernelGGL(exposure_forward_kernel<true>, dim3(nb), dim3(kExpBlock), 0, s, img, exposure, n, clamp, out);
    else
        hipLaunchKernelGGL(exposure_forward_kernel<false>, dim3(nb), dim3(kExpBlock), 0, s, img, exposure, n, clamp, out);
    return (int)hipGetLastError();
}

int gsr_exposure_backward(const float* img, const float* exposure, const float* dL_dout, int32_t H, int32_t W,
                          uint32_t flags, void* scratch, float* dL_dimg, float* dL_dexposure, void* stream) {
    if (int e = exposure_check(H, W, flags, !img || !exposure || !dL_dout || !scratch || !dL_dimg || !dL_dexposure))
        return e;
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return set_error(-1, "exposure: scratch must be 16-byte aligned");
    const long long n = (long long)H * W;
    const int nb = depth_loss_blocks(n), clamp = (flags & GSR_EXPOSURE_CLAMP) ? 1 : 0;
    float4* part = static_cast<float4*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    if (exposure_vec(n, {img, dL_dout, dL_dimg}))
        hipLaunchKernelGGL(exposure_backward_kernel<true>, dim3(nb), dim3(kExpBlock), 0, s, img, exposure, dL_dout, n,
                           clamp, dL_dimg, part);
    else
        hipLaunchKernelGGL(exposure_backward_kernel<false>, dim3(nb), dim3(kExpBlock), 0, s, img, exposure, dL_dout, n,
                           clamp, dL_dimg, part);
    hipLaunchKernelGGL(exposure_finalize_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const float*>(part), nb,
                       dL_dexposure);
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
        for (const void* p : {(const void*)g.param, (const void*)g.grad, (const void*)g.exp_avg, (const void*)g.exp_avg_sq})
            if (reinterpret_cast<uintptr_t>(p) & 15) return set_error(-1, "adam: tensors must be 16-byte aligned");
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
    if (reinterpret_cast<uintptr_t>(rot_raw) & 15) return set_error(-1, "mcmc_noise: rotations must be 16-byte aligned");
    for (const void* p : {(const void*)xyz, (const void*)scale_raw, (const void*)opac_raw, (const void*)noise})
        if (reinterpret_cast<uintptr_t>(p) & 3) return set_error(-1, "mcmc_noise: tensors must be 4-byte aligned");
    if (strength == 0.0f) return 0;  // a zero displacement: xyz keeps its bytes
    const long long want = ((long long)P + kNoiseBlock - 1) / kNoiseBlock;
    const int nb = (int)(want < kNoiseMaxBlocks ? want : kNoiseMaxBlocks);
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(nb), dim3(kNoiseBlock), 0, (hipStream_t)stream, xyz, scale_raw,
                       reinterpret_cast<const float4*>(rot_raw), opac_raw, noise, P, strength, guard_k, guard_cap);
    return (int)hipGetLastError();
}

int gsr_mcmc_relocate(const float* opacities, const float* scales, const int32_t* ratios, int32_t n, float min_opacity,
                      float* new_opacities, float* new_scales, void* stream) {
    if (n < 0) return set_error(-1, "mcmc_relocate: negative n");
    if (!(min_opacity > 0.0f && min_opacity < 1.0f)) return set_error(-1, "mcmc_relocate: min_opacity must lie in (0, 1)");
    if (n == 0) return 0;
    if (!opacities || !scales || !ratios || !new_opacities || !new_scales)
        return set_error(-1, "mcmc_relocate: null pointer");
    hipLaunchKernelGGL(mcmc_relocate_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, opacities, scales,
                       ratios, n, min_opacity, new_opacities, new_scales);
    return (int)hipGetLastError();
}

size_t gsr_compact_scratch_bytes(int32_t n) {
    const size_t nb = (size_t)((n > 0 ? n : 0) + kCmpPer - 1) / kCmpPer;
    return align256((nb + 1) * sizeof(int));
}

int gsr_compact_index(const uint8_t* mask, int32_t n, int32_t* idx_out, int32_t* count_out, void* scratch, void* stream) {
    if (n < 0) return set_error(-1, "compact: negative n");
    if (!count_out || !scratch || (n > 0 && (!mask || !idx_out))) return set_error(-1, "compact: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return (int)hipMemsetAsync(count_out, 0, sizeof(int32_t), s);
    const int nb = (n + kCmpPer - 1) / kCmpPer;
    int* counts = static_cast<int*>(scratch);
    hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(kCmpBlock), 0, s, mask, n, counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, counts, nb, count_out);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nb), dim3(kCmpBlock), 0, s, mask, n, counts, idx_out);
    return (int)hipGetLastError();
}

int gsr_gather_rows(const gsr_row_copy* copies, int32_t ncopies, const int32_t* idx, int32_t n_out, void* stream) {
    if (ncopies < 0 || ncopies > GSR_GATHER_MAX) return set_error(-1, "gather_rows: 0..24 copies");
    if (n_out < 0) return set_error(-1, "gather_rows: negative n_out");
    if (ncopies == 0 || n_out == 0) return 0;
    if (!copies || !idx) return set_error(-1, "gather_rows: null pointer");
    GatherArgs a;
    std::memset(&a, 0, sizeof a);
    long long maxw = 0;
    for (int i = 0; i < ncopies; ++i) {
        if (!copies[i].src || !copies[i].dst || copies[i].width <= 0) return set_error(-1, "gather_rows: bad copy");
        if (copies[i].src == copies[i].dst) return set_error(-1, "gather_rows: dst aliases src");
        a.c[i] = copies[i];
        maxw = copies[i].width > maxw ? copies[i].width : maxw;
    }
    const long long blocks = ((long long)n_out * maxw + 255) / 256;
    if (blocks > INT32_MAX) return set_error(-1, "gather_rows: too large");
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks, ncopies), dim3(256), 0, (hipStream_t)stream, a, idx,
                       n_out);
    return (int)hipGetLastError();
}

}  // extern "C"
