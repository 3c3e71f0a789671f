// gsr_gauss_dev.h -- the per-Gaussian projection chain, stated once for the three kernels that walk
// it: F1 (gsr_preprocess.hip, forward), B2 (gsr_preprocess_bwd.hip, leaf gradients) and the camera
// pass (gsr_camera_bwd.hip, camera gradients).  Device code only: helpers and small PODs, no kernel,
// no launcher; in an unnamed namespace, so each kernel file keeps its own internal copies.
//
// The chain (same formulas and operation order as oracle/gsr_oracle.c
// preprocess_one / preprocess_backward_one): quaternion (w,x,y,z) -> R -> L = R diag(mod s) ->
// Sigma = L L^T (src/utils/general_utils.cpp:24-37,91-97, src/scene/gaussian_model.cpp:23-24);
// view-space mean t = V p; clip-space mean through the homogeneous divide; the EWA Jacobian J(t) with
// the x/y terms clamped to the 1.3 tan(fov) guard band; T = J W; cov2D = T Sigma T^T + 0.3 I; the
// anti-aliasing coefficient sqrt(max(0.000025, det0 / det)); the real SH basis up to degree 3 and
// its derivatives w.r.t. the unit view direction; and the gradients back through each.
//
// Every sum keeps one order of additions, and the header is compiled under the including file's
// flags: F1 and B2 are both built -ffp-contract=off, so the values B2 recomputes (the SH clamp bits
// of a banded forward, r and coef under anti-aliasing) are F1's bit for bit -- the same text under
// the same flag.  The camera pass is tolerance-compared and keeps the default contraction.
#pragma once
#include "gsr_kernels.h"

namespace gsr {
namespace {

// ---- spherical harmonics ----
constexpr float kSH_C0 = 0.28209479177387814f;
constexpr float kSH_C1 = 0.4886025119029199f;
__constant__ float kSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                -1.0925484305920792f, 0.5462742152960396f};
__constant__ float kSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                -0.5900435899266435f};

// Unit view direction from the camera centre to the mean, and its length before normalising.
struct ViewDir {
    float x, y, z, len;
};
__device__ __forceinline__ ViewDir view_dir(const float* campos, float p0, float p1, float p2) {
    const float vx = p0 - campos[0], vy = p1 - campos[1], vz = p2 - campos[2];
    ViewDir d;
    d.len = sqrtf(vx * vx + vy * vy + vz * vz);
    d.x = vx / d.len;
    d.y = vy / d.len;
    d.z = vz / d.len;
    return d;
}

// Real SH basis (degree D <= 3) of the unit direction (x, y, z); entries past (D + 1)^2 are zero.
// GRAD: also its partial derivatives w.r.t. x, y and z as free variables (sh_dir_to_mean projects);
// without it dbx / dby / dbz are not touched.
template <bool GRAD>
__device__ __forceinline__ void sh_basis(int D, float x, float y, float z, float* basis, float* dbx = nullptr,
                                         float* dby = nullptr, float* dbz = nullptr) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        basis[k] = 0.f;
        if constexpr (GRAD) dbx[k] = dby[k] = dbz[k] = 0.f;
    }
    basis[0] = kSH_C0;
    if (D >= 1) {
        basis[1] = -kSH_C1 * y;
        basis[2] = kSH_C1 * z;
        basis[3] = -kSH_C1 * x;
        if constexpr (GRAD) {
            dby[1] = -kSH_C1; dbz[2] = kSH_C1; dbx[3] = -kSH_C1;
        }
    }
    if (D >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        basis[4] = kSH_C2[0] * xy;
        basis[5] = kSH_C2[1] * yz;
        basis[6] = kSH_C2[2] * (2.0f * zz - xx - yy);
        basis[7] = kSH_C2[3] * xz;
        basis[8] = kSH_C2[4] * (xx - yy);
        if constexpr (GRAD) {
            dbx[4] = kSH_C2[0] * y; dby[4] = kSH_C2[0] * x;
            dby[5] = kSH_C2[1] * z; dbz[5] = kSH_C2[1] * y;
            dbx[6] = kSH_C2[2] * -2.f * x; dby[6] = kSH_C2[2] * -2.f * y; dbz[6] = kSH_C2[2] * 4.f * z;
            dbx[7] = kSH_C2[3] * z; dbz[7] = kSH_C2[3] * x;
            dbx[8] = kSH_C2[4] * 2.f * x; dby[8] = kSH_C2[4] * -2.f * y;
        }
        if (D >= 3) {
            basis[9] = kSH_C3[0] * y * (3.0f * xx - yy);
            basis[10] = kSH_C3[1] * xy * z;
            basis[11] = kSH_C3[2] * y * (4.0f * zz - xx - yy);
            basis[12] = kSH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
            basis[13] = kSH_C3[4] * x * (4.0f * zz - xx - yy);
            basis[14] = kSH_C3[5] * z * (xx - yy);
            basis[15] = kSH_C3[6] * x * (xx - 3.0f * yy);
            if constexpr (GRAD) {
                dbx[9] = kSH_C3[0] * 6.f * xy; dby[9] = kSH_C3[0] * 3.f * (xx - yy);
                dbx[10] = kSH_C3[1] * yz; dby[10] = kSH_C3[1] * xz; dbz[10] = kSH_C3[1] * xy;
                dbx[11] = kSH_C3[2] * -2.f * xy; dby[11] = kSH_C3[2] * (4.f * zz - xx - 3.f * yy); dbz[11] = kSH_C3[2] * 8.f * yz;
                dbx[12] = kSH_C3[3] * -6.f * xz; dby[12] = kSH_C3[3] * -6.f * yz; dbz[12] = kSH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
                dbx[13] = kSH_C3[4] * (4.f * zz - 3.f * xx - yy); dby[13] = kSH_C3[4] * -2.f * xy; dbz[13] = kSH_C3[4] * 8.f * xz;
                dbx[14] = kSH_C3[5] * 2.f * xz; dby[14] = kSH_C3[5] * -2.f * yz; dbz[14] = kSH_C3[5] * (xx - yy);
                dbx[15] = kSH_C3[6] * 3.f * (xx - yy); dby[15] = kSH_C3[6] * -6.f * xy;
            }
        }
    }
}

// SH -> RGB: rgb (basis[0] * sh_dc on entry) plus the terms k0 <= k < k0 + N of the SH-rest row, each
// channel's sum in k order; rest[3 * (k - k0) + ch] is coefficient k of channel ch (a whole row with
// k0 = 1, N = 15, or one staged chunk of it).  nb = (D + 1)^2.
template <int N>
__device__ __forceinline__ void sh_accum(float (&rgb)[3], const float (&basis)[16], int k0, int nb, const float* rest) {
#pragma unroll
    for (int kk = 0; kk < N; ++kk) {
        const int k = k0 + kk;
        if (k < nb)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb[ch] = rgb[ch] + basis[k] * rest[3 * kk + ch];
    }
}

// ... and its end: the colour is max(r + 0.5, 0); returns whether the channel clamped (its gradient
// stops there).
__device__ __forceinline__ bool sh_clamp(float& r) {
    r = r + 0.5f;
    const bool clamped = r < 0.0f;
    r = fmaxf(r, 0.0f);
    return clamped;
}

// Gradient of the colour w.r.t. the direction's x, y, z from the SH-rest row `rest` and the colour
// gradient past the clamp, dres.  With DREST the row's own gradient basis[k] dres is written too
// (drest may be `rest` itself: each coefficient is read before it is overwritten; coefficients past
// the active degree get zeros); without it basis and drest are not read.
template <bool DREST>
__device__ __forceinline__ void sh_dir_grad(int nb, int M_rest, const float (&dbx)[16], const float (&dby)[16],
                                            const float (&dbz)[16], const float* rest, const float (&dres)[3],
                                            float& ddx, float& ddy, float& ddz, const float* basis = nullptr,
                                            float* drest = nullptr) {
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        if (k > M_rest) break;
        if (k < nb) {
            const float c0 = rest[3 * (k - 1) + 0], c1 = rest[3 * (k - 1) + 1], c2 = rest[3 * (k - 1) + 2];
            if constexpr (DREST) {
                drest[3 * (k - 1) + 0] = basis[k] * dres[0];
                drest[3 * (k - 1) + 1] = basis[k] * dres[1];
                drest[3 * (k - 1) + 2] = basis[k] * dres[2];
            }
            const float sdot = c0 * dres[0] + c1 * dres[1] + c2 * dres[2];
            ddx += dbx[k] * sdot;
            ddy += dby[k] * sdot;
            ddz += dbz[k] * sdot;
        } else if constexpr (DREST) {
            drest[3 * (k - 1) + 0] = 0.f;
            drest[3 * (k - 1) + 1] = 0.f;
            drest[3 * (k - 1) + 2] = 0.f;
        }
    }
}

// ... onto the tangent plane of the unit sphere and through the normalisation: the gradient w.r.t.
// the mean (w.r.t. campos it is the negative).
__device__ __forceinline__ void sh_dir_to_mean(const ViewDir& d, float ddx, float ddy, float ddz, float (&dmean)[3]) {
    const float dd = d.x * ddx + d.y * ddy + d.z * ddz;
    dmean[0] = (ddx - d.x * dd) / d.len;
    dmean[1] = (ddy - d.y * dd) / d.len;
    dmean[2] = (ddz - d.z * dd) / d.len;
}

// ---- covariance ----
// Sigma = L L^T, L = R(q) diag(smod s), as its upper triangle c3; R and the effective scales se are
// what the scale / rotation gradients need afterwards.
__device__ __forceinline__ void cov3d_from_scale_rot(const float4& q, float s0, float s1, float s2, float smod,
                                                     float (&R)[9], float (&se)[3], float (&c3)[6]) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    R[0] = 1.f - 2.f * (y * y + z * z);
    R[1] = 2.f * (x * y - r * z);
    R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z);
    R[4] = 1.f - 2.f * (x * x + z * z);
    R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y);
    R[7] = 2.f * (y * z + r * x);
    R[8] = 1.f - 2.f * (x * x + y * y);
    se[0] = smod * s0;
    se[1] = smod * s1;
    se[2] = smod * s2;
    float L[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) L[3 * i + j] = R[3 * i + j] * se[j];
    c3[0] = L[0] * L[0] + L[1] * L[1] + L[2] * L[2];
    c3[1] = L[0] * L[3] + L[1] * L[4] + L[2] * L[5];
    c3[2] = L[0] * L[6] + L[1] * L[7] + L[2] * L[8];
    c3[3] = L[3] * L[3] + L[4] * L[4] + L[5] * L[5];
    c3[4] = L[3] * L[6] + L[4] * L[7] + L[5] * L[8];
    c3[5] = L[6] * L[6] + L[7] * L[7] + L[8] * L[8];
}

// ---- means ----
// View-space mean t = V p.
__device__ __forceinline__ void view_mean(const float* V, float p0, float p1, float p2, float (&t)[3]) {
    t[0] = V[0] * p0 + V[4] * p1 + V[8] * p2 + V[12];
    t[1] = V[1] * p0 + V[5] * p1 + V[9] * p2 + V[13];
    t[2] = V[2] * p0 + V[6] * p1 + V[10] * p2 + V[14];
}

// Clip-space mean and the homogeneous divide's factor mw = 1 / (hw + 1e-7); NDC = (hx, hy) mw.
struct ClipMean {
    float hx, hy, hw, mw;
};
__device__ __forceinline__ ClipMean clip_mean(const float* Pm, float p0, float p1, float p2) {
    ClipMean h;
    h.hx = Pm[0] * p0 + Pm[4] * p1 + Pm[8] * p2 + Pm[12];
    h.hy = Pm[1] * p0 + Pm[5] * p1 + Pm[9] * p2 + Pm[13];
    h.hw = Pm[3] * p0 + Pm[7] * p1 + Pm[11] * p2 + Pm[15];
    h.mw = 1.0f / (h.hw + 0.0000001f);
    return h;
}

// ---- EWA projection ----
// cov2D = T Sigma T^T, T = J W: (a0, b, c0) before and (a, b, c) after the 0.3 px^2 dilation.
// t = (tx, ty, tz) is the view-space mean; (cx, cy) = its x, y clamped to the guard band; xmul / ymul
// are 0 outside it, else 1.  ST0 = Sigma T0^T, ST1 = Sigma T1^T (T0, T1 the rows of T) are kept for the
// gradients; Sigma is symmetric, so they are also the rows of T Sigma, term for term in the same k order.
struct Ewa {
    float tx, ty, tz, tz2;
    float fx, fy, cx, cy, xmul, ymul;
    float J00, J02, J11, J12;
    float T0[3], T1[3], ST0[3], ST1[3];
    float a0, b, c0, a, c, det;
};
__device__ __forceinline__ Ewa ewa_project(const gsr_camera& cam, const float (&t)[3], const float (&c3)[6]) {
    const float* V = cam.viewmatrix;
    Ewa E;
    E.tx = t[0];
    E.ty = t[1];
    E.tz = t[2];
    const float Wf = (float)cam.width, Hf = (float)cam.height;
    E.fx = Wf / (2.0f * cam.tanfovx);
    E.fy = Hf / (2.0f * cam.tanfovy);
    const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
    const float txtz = E.tx / E.tz, tytz = E.ty / E.tz;
    E.cx = fminf(limx, fmaxf(-limx, txtz)) * E.tz;
    E.cy = fminf(limy, fmaxf(-limy, tytz)) * E.tz;
    E.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    E.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    E.tz2 = E.tz * E.tz;
    E.J00 = E.fx / E.tz;
    E.J02 = -(E.fx * E.cx) / E.tz2;
    E.J11 = E.fy / E.tz;
    E.J12 = -(E.fy * E.cy) / E.tz2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        E.T0[k] = E.J00 * V[4 * k + 0] + E.J02 * V[4 * k + 2];
        E.T1[k] = E.J11 * V[4 * k + 1] + E.J12 * V[4 * k + 2];
    }
    const float S[9] = {c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        E.ST0[i] = S[3 * i + 0] * E.T0[0] + S[3 * i + 1] * E.T0[1] + S[3 * i + 2] * E.T0[2];
        E.ST1[i] = S[3 * i + 0] * E.T1[0] + S[3 * i + 1] * E.T1[1] + S[3 * i + 2] * E.T1[2];
    }
    E.a0 = E.ST0[0] * E.T0[0] + E.ST0[1] * E.T0[1] + E.ST0[2] * E.T0[2];
    E.a = E.a0 + 0.3f;
    E.b = E.ST0[0] * E.T1[0] + E.ST0[1] * E.T1[1] + E.ST0[2] * E.T1[2];
    E.c0 = E.ST1[0] * E.T1[0] + E.ST1[1] * E.T1[1] + E.ST1[2] * E.T1[2];
    E.c = E.c0 + 0.3f;
    E.det = E.a * E.c - E.b * E.b;
    return E;
}

// Anti-aliasing (GSR_FLAG_ANTIALIAS): the opacity compensation coef = sqrt(max(0.000025, r)),
// r = det(cov2D) / det(cov2D + 0.3 I).
__device__ __forceinline__ float aa_ratio(const Ewa& E) { return (E.a0 * E.c0 - E.b * E.b) / E.det; }
__device__ __forceinline__ float aa_coef(float r) { return sqrtf(fmaxf(0.000025f, r)); }

// ---- gradients ----
// conic (A, B, C) = inv([[a, b], [b, c]]): dL/d(a, b, c) from dL/d(A, B, C).
struct Cov2dGrad {
    float da, db, dc;
    float inv2;  // 1 / det^2
};
__device__ __forceinline__ Cov2dGrad cov2d_grad(const Ewa& E, float dA, float dB, float dC) {
    const float a = E.a, b = E.b, c = E.c;
    Cov2dGrad G;
    G.inv2 = 1.0f / (E.det * E.det);
    G.da = G.inv2 * (-c * c * dA + b * c * dB - b * b * dC);
    G.db = G.inv2 * (2.f * b * c * dA - (a * c + b * b) * dB + 2.f * a * b * dC);
    G.dc = G.inv2 * (-b * b * dA + a * b * dB - a * a * dC);
    return G;
}

// Anti-aliasing: the forward blended o' = o coef, and dLdo is dL/do'.  dL/dr = o dL/do' / (2 coef)
// (zero at the clamp) joins the cov2D gradients, with r's derivatives in their cancellation-free
// forms: (c0 det - det0 c) / det^2 = (h (c0^2 + b^2) + h^2 c0) / det^2.  Returns coef
// (dL/do = coef dL/do').
__device__ __forceinline__ float aa_cov2d_grad(const Ewa& E, float opac, float dLdo, Cov2dGrad& G) {
    const float a0 = E.a0, b = E.b, c0 = E.c0, inv2 = G.inv2;
    const float h = 0.3f;
    const float r = aa_ratio(E);
    const float coef = aa_coef(r);
    const float dL_dr = r <= 0.000025f ? 0.f : (opac * dLdo) / (2.f * coef);
    G.da += dL_dr * ((h * (c0 * c0 + b * b) + h * h * c0) * inv2);
    G.dc += dL_dr * ((h * (a0 * a0 + b * b) + h * h * a0) * inv2);
    G.db += dL_dr * (-2.f * b * (h * (a0 + c0) + h * h) * inv2);
    return coef;
}

// cov2D = T Sigma T^T: the gradients of the rows of T, and through T = J W those of J's entries.
struct TJGrad {
    float dT0[3], dT1[3];
    float dJ00, dJ02, dJ11, dJ12;
};
__device__ __forceinline__ TJGrad tj_grad(const Ewa& E, const float* V, const Cov2dGrad& G) {
    TJGrad d;
    d.dJ00 = d.dJ02 = d.dJ11 = d.dJ12 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d.dT0[i] = 2.f * E.ST0[i] * G.da + E.ST1[i] * G.db;
        d.dT1[i] = 2.f * E.ST1[i] * G.dc + E.ST0[i] * G.db;
        d.dJ00 += d.dT0[i] * V[4 * i + 0];
        d.dJ02 += d.dT0[i] * V[4 * i + 2];
        d.dJ11 += d.dT1[i] * V[4 * i + 1];
        d.dJ12 += d.dT1[i] * V[4 * i + 2];
    }
    return d;
}

}  // namespace
}  // namespace gsr
