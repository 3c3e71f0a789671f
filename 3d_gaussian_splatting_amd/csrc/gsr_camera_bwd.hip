// gsr_camera_bwd.hip -- the camera gradient: dL/dviewmatrix, dL/dprojmatrix and dL/dcampos from the
// per-Gaussian 2D gradients (grad2d, the hand-off between B1 and B2), on gfx950.
//
// The whole dependence of a render on the camera sits in the per-Gaussian preprocess, and the three
// camera fields of the ABI are read there as independent inputs:
//   viewmatrix  the view-space mean t = V p (EWA Jacobian J(t), depth channel v = tz or 1 / tz) and the
//               rotation rows of T = J W (cov2D = T Sigma T^T)
//   projmatrix  the NDC mean (hx, hy) / (hw + 1e-7); the 4k+2 entries are never read
//   campos      the SH view direction normalize(p - campos)
// One thread per Gaussian walks the chain B2 walks, through the same helpers (gsr_gauss_dev.h), up to
// dtx/dty/dtz, dT0/dT1, the homogeneous-divide terms and the direction gradient, and instead of
// chaining them to the mean it multiplies them with the other factor of each camera entry.
// 27 entries are live: viewmatrix 4k+r (r < 3), projmatrix 4k+{0,1,3}, campos.
//
// Reduction over P: registers, a wave64 butterfly, LDS across the block's four waves, one 27-float
// partial per block (stored sum-major); camera_finalize_kernel (one block per output entry) sums each
// sum's partials in double in a fixed order.
// The grid depends on P alone and nothing is atomic, so two calls give the same bits.
//
// Data movement is the cost (SH-rest rows: 180 of ~290 B per visible Gaussian at degree 3): the
// block's rows are staged through LDS by consecutive lanes reading consecutive addresses, rows of
// culled Gaussians skipped.  The SH clamp bits are the forward's stored ones (full images only).
#include "gsr_gauss_dev.h"
#include "gsr_kernels.h"

namespace gsr {
namespace {

constexpr int kCamSums = 27;  // acc[0..12): viewmatrix 4k+r at 3k+r; [12..24): projmatrix 4k+{0,1,3} at 12+3k+{0,1,2}; [24..27): campos

// depth_mode: 0 = colour only; 1 = grad2d slot 9 is dL/dz of the depth channel; 2 = dL/d(1/z).
// aa: the forward ran with GSR_FLAG_ANTIALIAS (grad2d slot 5 is dL/do').
// (at most 3 waves per SIMD: the staged rows' LDS admits three blocks per CU at degree 3 anyway, and the
// staging keeps 12 float4 loads in flight per thread, which must stay in registers)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 3))) void camera_backward_kernel(const CamArg<1> cams, const GaussIn in,
                                                              const uint32_t* __restrict__ depth_key,
                                                              const uint32_t* __restrict__ flags,
                                                              const float* __restrict__ grad2d, int depth_mode, int aa,
                                                              float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sh_lds[];
    __shared__ uint32_t vis_lds[256];
    __shared__ float red[4][kCamSums];
    const gsr_camera& cam = cams.c[0];
    const int P = in.P;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int M3 = in.M_rest * 3;
    const bool visible = g < P && depth_key[g] != 0xFFFFFFFFu;
    const bool stage = in.sh_rest != nullptr && !in.colors && in.D > 0;  // block-uniform
    float acc[kCamSums];
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) acc[k] = 0.f;

    // per-Gaussian inputs first: their latency overlaps the staging
    float g2[9], gz = 0.f, p[3] = {0.f, 0.f, 0.f}, c3[6], s3[3] = {0.f, 0.f, 0.f}, opac_in = 0.f;
    uint32_t cl = 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) g2[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) c3[k] = 0.f;
    if (visible) {
        const float4* src = reinterpret_cast<const float4*>(grad2d + (size_t)kPart * g);
        const float4 v0 = src[0], v1 = src[1], v2 = src[2];
        g2[0] = v0.x; g2[1] = v0.y; g2[2] = v0.z; g2[3] = v0.w;
        g2[4] = v1.x; g2[5] = v1.y; g2[6] = v1.z; g2[7] = v1.w;
        g2[8] = v2.x;
        gz = v2.y;
        p[0] = in.means3D[3 * (size_t)g + 0];
        p[1] = in.means3D[3 * (size_t)g + 1];
        p[2] = in.means3D[3 * (size_t)g + 2];
        if (in.cov3D) {
#pragma unroll
            for (int k = 0; k < 6; ++k) c3[k] = in.cov3D[6 * (size_t)g + k];
        } else {
            const float4 q = *reinterpret_cast<const float4*>(in.rots + 4 * (size_t)g);
            c3[0] = q.x; c3[1] = q.y; c3[2] = q.z; c3[3] = q.w;
            s3[0] = in.scales[3 * (size_t)g + 0];
            s3[1] = in.scales[3 * (size_t)g + 1];
            s3[2] = in.scales[3 * (size_t)g + 2];
        }
        if (!in.colors) cl = flags[g];
        if (aa) opac_in = in.opac[g];
    }
    if (stage) {
        // the block's 256 rows are one contiguous stretch of floats; element i belongs to row i / M3
        vis_lds[threadIdx.x] = visible ? 1u : 0u;
        __syncthreads();
        const int rows = P - blockIdx.x * 256 < 256 ? P - blockIdx.x * 256 : 256;
        const size_t base = (size_t)blockIdx.x * 256 * M3;
        const int nf = rows * M3;
        const float* __restrict__ src = in.sh_rest + base;
        int done = 0;  // floats staged by the 16-B form
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
            // 16 B per lane, and every load of the thread issued before the first LDS store, so that a
            // block pays one memory latency for its rows, not one per 1 KB (M3 <= 45: <= 12 per thread).
            // Piece j holds floats 4j .. 4j+3, of rows `row` and possibly row + 1: loaded if either is visible.
            const int nf4 = nf >> 2;
            const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
            float4* lds4 = reinterpret_cast<float4*>(sh_lds);
            const int qs = 1024 / M3, rs = 1024 % M3;  // row and remainder advance per 256 pieces
            int row = (4 * (int)threadIdx.x) / M3, rem = (4 * (int)threadIdx.x) % M3;
            float4 v[12];
            uint32_t got = 0u;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const int j = threadIdx.x + 256 * k;
                // no divergent branch around the load (it would make each load wait for the one before):
                // a lane with nothing to fetch re-reads the block's piece 0, which costs no HBM traffic
                const int r0 = row < 255 ? row : 255, r1 = rem + 3 >= M3 && row < 255 ? row + 1 : r0;
                const bool ld = (j < nf4) & ((vis_lds[r0] | vis_lds[r1]) != 0u);
                v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (256 * k < nf4) v[k] = src4[ld ? j : 0];  // block-uniform condition
                got |= (ld ? 1u : 0u) << k;
                row += qs;
                rem += rs;
                if (rem >= M3) {
                    rem -= M3;
                    ++row;
                }
            }
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (got & (1u << k)) lds4[threadIdx.x + 256 * k] = v[k];
            done = nf4 << 2;
        }
        // the 4-B form: everything when the rows do not start 16-B aligned, else the last nf % 4 floats
        for (int i = done + threadIdx.x; i < nf; i += 256)
            if (vis_lds[i / M3]) sh_lds[i] = src[i];
        __syncthreads();
    }
    if (visible) {
        const float* V = cam.viewmatrix;
        const float* Pm = cam.projmatrix;
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        // ---- campos, through the SH view direction ----
        if (stage) {
            const float* rest = sh_lds + threadIdx.x * M3;
            const int D = in.D, nb = (D + 1) * (D + 1);
            const ViewDir d = view_dir(cam.campos, p0, p1, p2);
            float basis[16], dbx[16], dby[16], dbz[16];  // the basis itself is not used here
            sh_basis<true>(D, d.x, d.y, d.z, basis, dbx, dby, dbz);
            const float dres[3] = {(cl & 1u) ? 0.f : g2[6], (cl & 2u) ? 0.f : g2[7], (cl & 4u) ? 0.f : g2[8]};
            float ddx = 0.f, ddy = 0.f, ddz = 0.f;
            sh_dir_grad<false>(nb, in.M_rest, dbx, dby, dbz, rest, dres, ddx, ddy, ddz);
            float dmv[3];
            sh_dir_to_mean(d, ddx, ddy, ddz, dmv);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[24 + k] = -dmv[k];  // the direction is p - campos
        }
        // ---- projmatrix, through the NDC mean ----
        {
            const ClipMean h = clip_mean(Pm, p0, p1, p2);
            const float hx = h.hx, hy = h.hy, mw = h.mw;
            const float dhx = mw * g2[0], dhy = mw * g2[1];
            const float dhw = -(hx * g2[0] + hy * g2[1]) * (mw * mw);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float pk = k < 3 ? p[k] : 1.f;
                acc[12 + 3 * k + 0] = dhx * pk;
                acc[12 + 3 * k + 1] = dhy * pk;
                acc[12 + 3 * k + 2] = dhw * pk;
            }
        }
        // ---- viewmatrix: conic -> cov2D -> T = J W and the view-space mean ----
        if (!in.cov3D) {
            float R[9], se[3];
            cov3d_from_scale_rot(make_float4(c3[0], c3[1], c3[2], c3[3]), s3[0], s3[1], s3[2], in.smod, R, se, c3);
        }
        float t[3];
        view_mean(V, p0, p1, p2, t);
        const Ewa E = ewa_project(cam, t, c3);
        Cov2dGrad G = cov2d_grad(E, g2[2], g2[3], g2[4]);
        if (aa) aa_cov2d_grad(E, opac_in, g2[5], G);  // the chain through coef
        const TJGrad dj = tj_grad(E, V, G);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            // T0_i = J00 V[4i] + J02 V[4i+2], T1_i = J11 V[4i+1] + J12 V[4i+2]
            acc[3 * i + 0] = dj.dT0[i] * E.J00;
            acc[3 * i + 1] = dj.dT1[i] * E.J11;
            acc[3 * i + 2] = dj.dT0[i] * E.J02 + dj.dT1[i] * E.J12;
        }
        const float tz2 = E.tz2, tz3 = tz2 * E.tz, fx = E.fx, fy = E.fy;
        // Outside the guard band cx = +-limx tz, so J02 = -+fx limx / tz and dJ02/dtz = fx cx / tz^3: half
        // the in-band 2 fx cx / tz^3.  B2 keeps upstream's in-band factor for both (it treats a clamped cx
        // as a constant); here the forward's own derivative is taken, which is what float64 autograd of
        // the forward gives.
        const float dt[3] = {E.xmul * (-fx / tz2) * dj.dJ02, E.ymul * (-fy / tz2) * dj.dJ12,
                             (-fx / tz2) * dj.dJ00 + (-fy / tz2) * dj.dJ11 + ((1.f + E.xmul) * fx * E.cx / tz3) * dj.dJ02 +
                                 ((1.f + E.ymul) * fy * E.cy / tz3) * dj.dJ12 +
                                 (depth_mode == 1 ? gz : depth_mode == 2 ? -gz / tz2 : 0.f)};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[0 + r] += dt[r] * p0;
            acc[3 + r] += dt[r] * p1;
            acc[6 + r] += dt[r] * p2;
            acc[9 + r] = dt[r];
        }
    }
    // ---- block sum: wave64 butterfly, then the four waves in a fixed order ----
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kCamSums; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    // sum k of every block is one contiguous row of the scratch: the finalize reads it coalesced
    if (threadIdx.x < kCamSums)
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The finalize: one block of 256 threads per output entry (36 blocks), so no thread carries more than
// one sum and nothing is shuffled 27 times over.  Block e adds its sum's row of the scratch
// (part[k * nparts + block], read coalesced) in double -- each thread its elements in index order, then a
// fixed tree across the threads -- and writes (not accumulates) entry e; the entries no kernel reads are
// written as zeros.  (One block for all 27 sums is a latency chain on one CU: 16 rounds of 27 strided
// loads per thread, or with 1024 threads 27 x 6 double shuffles in each of 16 waves through one LDS.)
__global__ __launch_bounds__(256) void camera_finalize_kernel(const float* __restrict__ part, int nparts,
                                                              float* __restrict__ dcam) {
    __shared__ double r[4];
    const int e = blockIdx.x;  // output entry -> its sum (or none)
    int k = -1;
    if (e < 16) {
        if ((e & 3) < 3) k = 3 * (e >> 2) + (e & 3);
    } else if (e < 32) {
        const int c = (e - 16) & 3;
        if (c != 2) k = 12 + 3 * ((e - 16) >> 2) + (c == 3 ? 2 : c);
    } else if (e < 35) {
        k = 24 + (e - 32);
    }
    if (k < 0) {  // block-uniform
        if (threadIdx.x == 0) dcam[e] = 0.f;
        return;
    }
    const float* __restrict__ row = part + (size_t)k * nparts;
    double s = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < nparts; i += 256) s += (double)row[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dcam[e] = (float)((r[0] + r[1]) + (r[2] + r[3]));
}

}  // namespace

size_t camera_grad_scratch_bytes(long long P) {
    const long long blocks = P > 0 ? div_up(P, 256) : 1;
    return ((size_t)blocks * kCamSums * sizeof(float) + 15) & ~(size_t)15;
}

int launch_camera_backward(const gsr_camera& cam, const GaussIn& in, const uint32_t* depth_key, const uint32_t* flags,
                           const float* grad2d, int depth_mode, bool aa, float* part, float* dcam, hipStream_t s) {
    const int blocks = in.P > 0 ? div_up(in.P, 256) : 0;
    if (blocks > 0) {
        const bool stage = in.sh_rest && !in.colors && in.D > 0;
        const size_t lds = stage ? sizeof(float) * 256 * 3 * in.M_rest : 0;
        const CamArg<1> c1{{cam}};
        hipLaunchKernelGGL(camera_backward_kernel, dim3(blocks), dim3(256), lds, s, c1, in, depth_key, flags, grad2d,
                           depth_mode, aa ? 1 : 0, part);
        if (int e = (int)hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(camera_finalize_kernel, dim3(GSR_CAMERA_GRAD_FLOATS), dim3(256), 0, s, part, blocks, dcam);
    return (int)hipGetLastError();
}

}  // namespace gsr
