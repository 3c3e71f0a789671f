// gsr_pointset.hip -- the refinement-time edits of the point set (include/gsr/gsr_train.h) on
// gfx950: they run when Gaussians are pruned, cloned, split or relocated, not per iteration.
//
//  * compact_count / compact_scan / compact_scatter_kernel  mask -> ascending index list (wave64
//                         ballot counts, block-local scan).
//  * gather_rows_kernel   a multi-tensor row gather (prune / clone), one launch for up to
//                         GSR_GATHER_MAX tensors.
//  * mcmc_relocate_kernel the opacity / scale a relocated Gaussian and its copies take: the
//                         binomial sum in fp64, one thread per sampled row.
#include <climits>
#include <cstring>

#include "gsr/gsr_train.h"
#include "gsr_train_dev.h"

namespace gsr {
namespace {

// ---------------------------------------------------------------- MCMC relocation
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

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

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
