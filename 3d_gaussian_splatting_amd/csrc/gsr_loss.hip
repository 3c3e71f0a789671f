// gsr_loss.hip -- the image-plane kernels of the training step (include/gsr/gsr_train.h,
// SURVEY.md §8f row 1) on gfx950.
//
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
//                         float4 per thread, one (sum |e|, count) partial per block.
//  * exposure_*_kernel    the trained per-view 3 x 4 colour transform on the render (upstream's
//                         use_trained_exp) and its adjoint: 4 pixels of all three planes per thread,
//                         dL/dimg and one 12-float partial of dL/dexposure per block.
//  * loss_finalize_kernel, depth_loss_finalize_kernel, exposure_finalize_kernel  the per-block
//                         partials summed in double by one block (finalize_partials: fixed order, no
//                         atomics), each with its own epilogue.
#include <cmath>

#include "gsr/gsr_train.h"
#include "gsr_train_dev.h"

namespace gsr {
namespace {

// ---------------------------------------------------------------- SSIM + L1
constexpr int kWin = 11, kRad = 5;
constexpr int kTX = 64, kTY = 16;                              // output tile
constexpr int kRX = kTX + 2 * kRad, kRY = kTY + 2 * kRad;      // 74 x 26 staged tile
constexpr int kRXP = kRX + 1;                                  // LDS row pitch
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct Window {
    float w[kWin];
};

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
    __shared__ double r[2][256];  // sum S | sum |x - y|
    finalize_partials(&part->x, nparts, r);
    if (threadIdx.x == 0) {
        const float ssim = (float)(r[0][0] * inv_n), l1 = (float)(r[1][0] * inv_n);
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
// does not depend on the sum), as a plane stream (gsr_train_dev.h).
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

// the pixels e0 .. e0 + cnt - 1 of one thread: gradients out, (sum |e|, count) into the thread's sums
template <bool V4>
__device__ __forceinline__ void depth_loss_group(const DepthLossArgs& a, long long e0, int cnt, float& asum,
                                                 float& cnt_sum) {
#pragma clang fp contract(off)  // both instantiations round alike: float4 and scalar paths, same bits
    const bool norm = a.mode == GSR_DEPTH_NORMALIZED;
    float d[4], t[4], m[4], al[4] = {0.f, 0.f, 0.f, 0.f}, gd[4], ga[4];
    load4<V4>(a.depth, e0, cnt, d);
    load4<V4>(a.target, e0, cnt, t);
    if (a.mask) {
        load4<V4>(a.mask, e0, cnt, m);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = k < cnt ? 1.f : 0.f;
    }
    if (norm) load4<V4>(a.alpha, e0, cnt, al);
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
    store4<V4>(a.d_depth, e0, cnt, gd);
    if (norm) store4<V4>(a.d_alpha, e0, cnt, ga);
}

template <bool VEC>
__global__ __launch_bounds__(kPlaneBlock) void depth_loss_kernel(const DepthLossArgs a, float2* __restrict__ part) {
    __shared__ float red[8];
    float asum = 0.f, cnt_sum = 0.f;
    for_each_plane_group<VEC>(a.n, [&](auto v4, long long e0, int cnt) {
        depth_loss_group<decltype(v4)::value>(a, e0, cnt, asum, cnt_sum);
    });
    block_sum2(asum, cnt_sum, red);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(asum, cnt_sum);
}

__global__ __launch_bounds__(256) void depth_loss_finalize_kernel(const float2* __restrict__ part, int nparts,
                                                                  double inv_n, float weight,
                                                                  float* __restrict__ stats) {
    __shared__ double r[2][256];  // sum |e| | count
    finalize_partials(&part->x, nparts, r);
    if (threadIdx.x == 0) {
        const float l1 = (float)(r[0][0] * inv_n);
        stats[0] = weight * l1;
        stats[1] = l1;
        stats[2] = (float)r[1][0];
    }
}

// ---------------------------------------------------------------- per-view exposure
// out = clamp?(x E[:3,:3] + E[:3,3]) over a channel-major 3 x H x W image (x a row vector per pixel,
// so the 3 x 3 part is indexed E[i][j]: input channel i, output channel j), and its adjoint, as
// plane streams over the H * W pixels (gsr_train_dev.h).
constexpr int kExpWaves = kPlaneBlock / 64;

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
    for (int i = 0; i < 3; ++i) load4<V4>(img + i * n, e0, cnt, x[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = exposure_y(E, j, x[0][k], x[1][k], x[2][k]);
            y[k] = clamp ? fminf(fmaxf(v, 0.f), 1.f) : v;
        }
        store4<V4>(out + j * n, e0, cnt, y);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPlaneBlock) void exposure_forward_kernel(const float* __restrict__ img,
                                                                       const float* __restrict__ exposure, long long n,
                                                                       int clamp, float* __restrict__ out) {
    float E[12];
    exposure_load_matrix(exposure, E);
    for_each_plane_group<VEC>(n, [&](auto v4, long long e0, int cnt) {
        exposure_forward_group<decltype(v4)::value>(img, out, E, n, e0, cnt, clamp != 0);
    });
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
        load4<V4>(img + i * n, e0, cnt, x[i]);
        load4<V4>(dout + i * n, e0, cnt, g[i]);
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
        store4<V4>(dimg + i * n, e0, cnt, d);
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
__global__ __launch_bounds__(kPlaneBlock) void exposure_backward_kernel(const float* __restrict__ img,
                                                                        const float* __restrict__ exposure,
                                                                        const float* __restrict__ dout, long long n,
                                                                        int clamp, float* __restrict__ dimg,
                                                                        float4* __restrict__ part) {
    __shared__ float red[kExpWaves][12];
    float E[12], acc[12];
    exposure_load_matrix(exposure, E);
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    for_each_plane_group<VEC>(n, [&](auto v4, long long e0, int cnt) {
        exposure_backward_group<decltype(v4)::value>(img, dout, dimg, E, n, e0, cnt, clamp != 0, acc);
    });
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

// the sums written (not accumulated) into the 3 x 4 layout of the parameter
__global__ __launch_bounds__(256) void exposure_finalize_kernel(const float* __restrict__ part, int nparts,
                                                                float* __restrict__ dexposure) {
    __shared__ double r[12][256];
    finalize_partials(part, nparts, r);
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;  // k < 9: sum x_i g_j at [i][j]; k = 9 + j: sum g_j at [j][3]
        dexposure[k < 9 ? 4 * (k / 3) + k % 3 : 4 * (k - 9) + 3] = (float)r[k][0];
    }
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

int check_image(const float* img, const float* gt, int C, int H, int W) {
    if (!img || !gt) return set_error(-1, "loss: null image");
    if (C <= 0 || H <= 0 || W <= 0) return set_error(-1, "loss: bad image shape");
    return 0;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

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
    return align256((size_t)plane_blocks(n) * sizeof(float2));
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
    // the ABI takes any 4-byte-aligned plane; float4 accesses need all of them at 16
    const bool vec = all_aligned16({a.depth, a.alpha, a.target, a.mask, a.d_depth, a.d_alpha});
    float2* part = static_cast<float2*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    launch_plane(vec, depth_loss_kernel<true>, depth_loss_kernel<false>, a.n, s, a, part);
    hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3(1), dim3(256), 0, s, part, plane_blocks(a.n), 1.0 / (double)a.n,
                       weight, stats);
    return (int)hipGetLastError();
}

size_t gsr_exposure_scratch_bytes(int32_t H, int32_t W) {
    const long long n = (long long)(H > 0 ? H : 0) * (W > 0 ? W : 0);
    return align256((size_t)plane_blocks(n) * 12 * sizeof(float));
}

// the checks both exposure passes share; 0, or < 0 with the error text set
static int exposure_check(int32_t H, int32_t W, uint32_t flags, bool any_null) {
    if (H <= 0 || W <= 0) return set_error(-1, "exposure: bad image shape");
    if (any_null) return set_error(-1, "exposure: null pointer");
    if (flags & ~(uint32_t)GSR_EXPOSURE_CLAMP) return set_error(-1, "exposure: unknown flag bits");
    return 0;
}

// In both passes float4 accesses need every plane at 16 bytes: an aligned base (all_aligned16 of
// the images) and a plane of a multiple of 4 pixels (n % 4 == 0).
int gsr_exposure_forward(const float* img, const float* exposure, int32_t H, int32_t W, uint32_t flags, float* out,
                         void* stream) {
    if (int e = exposure_check(H, W, flags, !img || !exposure || !out)) return e;
    const long long n = (long long)H * W;
    const int clamp = (flags & GSR_EXPOSURE_CLAMP) ? 1 : 0;
    launch_plane(n % 4 == 0 && all_aligned16({img, out}), exposure_forward_kernel<true>, exposure_forward_kernel<false>, n,
                 (hipStream_t)stream, img, exposure, n, clamp, out);
    return (int)hipGetLastError();
}

int gsr_exposure_backward(const float* img, const float* exposure, const float* dL_dout, int32_t H, int32_t W,
                          uint32_t flags, void* scratch, float* dL_dimg, float* dL_dexposure, void* stream) {
    if (int e = exposure_check(H, W, flags, !img || !exposure || !dL_dout || !scratch || !dL_dimg || !dL_dexposure))
        return e;
    if (!all_aligned16({scratch})) return set_error(-1, "exposure: scratch must be 16-byte aligned");
    const long long n = (long long)H * W;
    const int clamp = (flags & GSR_EXPOSURE_CLAMP) ? 1 : 0;
    float4* part = static_cast<float4*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    launch_plane(n % 4 == 0 && all_aligned16({img, dL_dout, dL_dimg}), exposure_backward_kernel<true>,
                 exposure_backward_kernel<false>, n, s, img, exposure, dL_dout, n, clamp, dL_dimg, part);
    hipLaunchKernelGGL(exposure_finalize_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const float*>(part),
                       plane_blocks(n), dL_dexposure);
    return (int)hipGetLastError();
}

}  // extern "C"
