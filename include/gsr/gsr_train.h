/*
 * gsr_train.h -- C ABI of the training-step kernels around the rasterizer (SURVEY.md §8f
 * rows 1-2): photometric loss, fused Adam over the six parameter groups, densification
 * statistics and the prune compaction.  Same conventions as gsr.h: caller-owned DEVICE
 * memory (f32, contiguous, channel-major images), one hipStream_t, 0 = ok / < 0 = error with
 * the message in gsr_last_error of gsr.h, no persistent allocations.
 *
 * What each entry point replaces in the reference (seiya-kumada/3d_gaussian_splatting):
 *
 *   gsr_activate           <- GaussianModel::get_scaling / get_rotation / get_opacity
 *                             (src/scene/gaussian_model.cpp:270-280,295-298; activations
 *                             exp / normalize / sigmoid bound at :54-58)
 *   gsr_loss_forward       <- the loss the training loop at src/utils/train_utils.cpp:128-145
 *   gsr_loss_backward         would compute: (1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM),
 *                             lambda_dssim from OptimizationParams (src/arguments/params.h:62).
 *                             The reference has no loss code (its loop is a stub); the
 *                             definition is the upstream 3DGS one (11x11 Gaussian window,
 *                             sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean).
 *   gsr_depth_loss         <- upstream 3DGS's depth regulariser (train.py: Ll1depth =
 *                             depth_l1_weight(iteration) * mean |(invDepth - mono_invdepth) *
 *                             depth_mask|) on the rasterizer's depth / alpha outputs
 *                             (gsr_forward_aux of gsr.h), value and gradients in one pass.  The
 *                             reference has no depth term; the normalised mode (depth / alpha)
 *                             is this project's addition.
 *   gsr_exposure_scratch_bytes <- upstream 3DGS's trained per-image exposure (gaussian_renderer/
 *   gsr_exposure_forward         __init__.py, use_trained_exp: matmul(image.permute(1,2,0),
 *   gsr_exposure_backward        exposure[:3,:3]).permute(2,0,1) + exposure[:3,3,None,None]) and the
 *                             backward autograd derives from it, one fused pass per direction.  The
 *                             reference has none.
 *   gsr_adam_step          <- the six torch::optim::Adam instances of GaussianModel::setup
 *                             (src/scene/gaussian_model.cpp:323-345: default AdamOptions,
 *                             betas 0.9 / 0.999, eps 1e-8, no weight decay) stepped once each,
 *                             with the activation backward (exp / sigmoid / normalize) of
 *                             the getters fused in front of the moment update.
 *   gsr_adam_step_sparse   <- upstream 3DGS's optimizer_type = "sparse_adam" (the reference has
 *                             none): the same step for the Gaussians the view rendered only.
 *   gsr_densify_stats      <- max_radii2D_ / xyz_gradient_accum_ / denom_ updates
 *                             (src/scene/gaussian_model.h:18-20; setup :318-319)
 *   gsr_compact_index      <- the boolean-mask selection of prune_points / densify_and_clone
 *   gsr_gather_rows           (upstream densification; the reference declares only the stats
 *                             tensors): index list from a mask, then one multi-tensor row
 *                             gather for parameters, Adam moments and statistics.
 *   gsr_mcmc_noise         <- gsplat's inject_noise_to_position (MCMCStrategy, "3D Gaussian Splatting
 *                             as Markov Chain Monte Carlo", Kheradmand et al. 2024): the per-step,
 *                             covariance-shaped, opacity-gated noise on the means, with the
 *                             activations and the covariance fused in.  Neither upstream 3DGS nor
 *                             the reference has it.
 *   gsr_mcmc_relocate      <- gsplat's `relocation` kernel (compute_relocation): the opacity and
 *                             scale that a Gaussian and the copies teleported onto it take so that
 *                             together they render as the one did.  Neither upstream 3DGS nor the
 *                             reference has it.
 */
#ifndef GSR_GSR_TRAIN_H
#define GSR_GSR_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exp / normalize / sigmoid of the raw leaves (GaussianModel getters).  Any output may be
 * NULL (skipped).  rot_raw / rot rows of 4 (w first), 16-B aligned. */
int gsr_activate(const float* scale_raw, const float* rot_raw, const float* opac_raw, int32_t P,
                 float* scales, float* rots, float* opacs, void* stream);

/* Loss over C x H x W images: stats[0] = loss, stats[1] = mean |img - gt|, stats[2] = mean SSIM
 * (device floats).  `maps` is caller scratch of gsr_loss_scratch_bytes(C, H, W) bytes holding
 * the per-pixel SSIM derivative maps for gsr_loss_backward.  Deterministic (fixed-order sums). */
size_t gsr_loss_scratch_bytes(int32_t C, int32_t H, int32_t W);
int gsr_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                     float lambda_dssim, void* maps, float* stats, void* stream);
/* dL/dimg (C x H x W) for dL/dloss = 1, from the maps the forward left in `maps`. */
int gsr_loss_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                      float lambda_dssim, const void* maps, float* dL_dimg, void* stream);

/* Depth L1 over an H x W plane (n = H * W pixels), for the depth / alpha outputs of
 * gsr_forward_aux.  With m = mask[i] (1 when mask is NULL) and e = (pred - target) * m:
 *   stats[0] = weight * mean_n |e|, stats[1] = mean_n |e|, stats[2] = the number of contributing
 *   pixels (m != 0, and alpha >= alpha_min in normalised mode; exact up to 2^24).  The mean
 *   divides by n, as upstream's .mean() does, not by the contributing count.
 * Gradients for dL/dloss = 1, written for every pixel: dL/dpred = (weight / n) m sign(e), sign(0) = 0;
 *   RAW         dL_ddepth = dL/dpred
 *   NORMALIZED  dL_ddepth = dL/dpred / alpha, dL_dalpha = -dL/dpred depth / alpha^2; both 0 (and
 *               the pixel contributes nothing) where alpha < alpha_min.
 * alpha / dL_dalpha: required in NORMALIZED mode, ignored (may be NULL) in RAW mode.  alpha_min
 * > 0 in NORMALIZED mode; weight finite and >= 0.  Planes: any 4-byte-aligned pointer (float4
 * accesses when all are 16-byte aligned).  scratch: gsr_depth_loss_scratch_bytes(H, W) bytes,
 * 8-byte aligned.  One pass plus a one-block finalize; deterministic (fixed-order sums, no atomics). */
#define GSR_DEPTH_RAW 0         /* pred = depth           (upstream: the un-normalised blend)   */
#define GSR_DEPTH_NORMALIZED 1  /* pred = depth / alpha   where alpha >= alpha_min; other pixels contribute nothing */
size_t gsr_depth_loss_scratch_bytes(int32_t H, int32_t W);
int gsr_depth_loss(const float* depth, const float* alpha, const float* target, const float* mask,
                   int32_t H, int32_t W, float weight, int32_t mode, float alpha_min,
                   void* scratch, float* stats, float* dL_ddepth, float* dL_dalpha, void* stream);

/* Per-view exposure: a 3 x 4 affine colour transform E (row-major, 12 DEVICE floats -- one row of
 * upstream's (N, 3, 4) parameter; it is a trained value and the host never reads it) applied to a
 * channel-major 3 x H x W image.  The 3 x 3 part multiplies the pixel as a ROW vector, so for output
 * channel j:
 *   y_j = E[0][j] x_0 + E[1][j] x_1 + E[2][j] x_2 + E[j][3]          (E[i][j], not E[j][i])
 *   out_j = y_j, or min(max(y_j, 0), 1) with GSR_EXPOSURE_CLAMP.
 * Backward, with g_j = dL_dout_j, and with the flag g_j = 0 where y_j < 0 or y_j > 1 (the bounds
 * are inclusive, as in torch.clamp: the gradient passes where y_j is exactly 0 or 1):
 *   dL_dimg_i = sum_j E[i][j] g_j;  dL_dexposure[i][j] = sum_p x_i g_j;  dL_dexposure[j][3] = sum_p g_j.
 * dL_dexposure (12 floats, may point into a larger gradient tensor) is WRITTEN, not accumulated.
 * The backward recomputes y with the forward's expression, so its mask is the forward's clamp.
 * Images: any 4-byte-aligned pointer (float4 accesses when every plane is 16-byte aligned).
 * scratch: gsr_exposure_scratch_bytes(H, W) bytes, 16-byte aligned.  The buffers must not overlap
 * (not checked).  One pass per direction plus a one-block finalize; deterministic (fixed-order
 * sums on a grid that depends on H * W alone, no atomics). */
#define GSR_EXPOSURE_CLAMP 1u   /* out = min(max(y, 0), 1) after the affine map (upstream's render clamps) */
size_t gsr_exposure_scratch_bytes(int32_t H, int32_t W);
int gsr_exposure_forward(const float* img, const float* exposure, int32_t H, int32_t W, uint32_t flags,
                         float* out, void* stream);
int gsr_exposure_backward(const float* img, const float* exposure, const float* dL_dout, int32_t H, int32_t W,
                          uint32_t flags, void* scratch, float* dL_dimg, float* dL_dexposure, void* stream);

/* Activation applied by the getter in front of a parameter group (its gradient arrives with
 * respect to the activated value; gsr_adam_step converts it to the raw leaf first). */
#define GSR_ACT_NONE 0       /* xyz, features_dc, features_rest */
#define GSR_ACT_EXP 1        /* scaling */
#define GSR_ACT_SIGMOID 2    /* opacity */
#define GSR_ACT_NORMALIZE4 3 /* rotation: rows of 4, x / max(|x|, 1e-12) */

typedef struct gsr_adam_group {
    float* param;            /* raw leaf, n floats (updated in place) */
    const float* grad;       /* gradient w.r.t. the ACTIVATED value (n floats) */
    float* exp_avg;          /* Adam state, n floats */
    float* exp_avg_sq;       /* Adam state, n floats */
    int64_t n;
    int32_t act;             /* GSR_ACT_* */
    int32_t step;            /* this group's step count AFTER increment (>= 1) */
    float lr;
} gsr_adam_group;
#define GSR_ADAM_MAX_GROUPS 8
/* One Adam step (libtorch torch::optim::Adam semantics, amsgrad off, weight_decay 0) of up
 * to GSR_ADAM_MAX_GROUPS groups in ONE launch; `groups` is a HOST array. */
int gsr_adam_step(const gsr_adam_group* groups, int32_t ngroups, float beta1, float beta2, float eps,
                  void* stream);
/* The same step behind a device-side guard: it is skipped ON THE DEVICE when
 * *guard_k > guard_cap (guard_k NULL: never skipped).  guard_k is the forward's instance count K
 * (gsr_view(GSR_VIEW_COUNTS) word 0, the scan's counter: the true K, not clamped) and guard_cap
 * the max_rendered bound that render ran under.  A render above its bound was truncated; a
 * training loop that renders without a per-iteration host read of K passes them so that the
 * truncated iteration's update is dropped instead of applied (the groups' step counts the host
 * already advanced are not rolled back). */
int gsr_adam_step_guarded(const gsr_adam_group* groups, int32_t ngroups, float beta1, float beta2, float eps,
                          const uint32_t* guard_k, uint32_t guard_cap, void* stream);
/* The visibility-masked ("sparse") step: the groups are rows of n / P floats per Gaussian, and only
 * the rows of Gaussians with radii[i] > 0 (device int32, P entries: the rasterizer's radii, the
 * rule of gsr_densify_stats) are stepped.  A visible row is updated exactly as gsr_adam_step
 * updates it -- same operations, same fused activation backward, bias corrections from the
 * group's `step` -- and comes out bit-identical to it.  A row with radii[i] <= 0 keeps the bytes
 * of param / exp_avg / exp_avg_sq and is not fetched; its grad is never used (it may hold
 * anything, NaN included).  The groups' step counts advance once per call as for the dense
 * step; no per-Gaussian step count is kept.  This is NOT the arithmetic of upstream 3DGS's
 * sparse_adam optimizer: libtorch's bias correction is kept, so that the all-visible step is the
 * dense step and the fused and the libtorch step stay interchangeable on one AdamParamState.
 * A group with n == 0 is skipped; n % P != 0 is an error, as is a GSR_ACT_NORMALIZE4 group whose
 * row is no multiple of 4 floats.  P == 0 or ngroups == 0: nothing to do, returns 0.  One launch,
 * no host read, no scratch; guard_k / guard_cap as gsr_adam_step_guarded (NULL: never skipped). */
int gsr_adam_step_sparse(const gsr_adam_group* groups, int32_t ngroups, const int32_t* radii, int32_t P,
                         float beta1, float beta2, float eps, const uint32_t* guard_k, uint32_t guard_cap,
                         void* stream);

/* Densification statistics for the visible Gaussians (radii > 0):
 *   max_radii2D = max(max_radii2D, radii); grad_accum += |dL/dmeans2D[:, :2]|; denom += 1.
 * dmeans2D: P x 3 (the rasterizer's dL_dmeans2D, the reference's viewspace_points grad). */
int gsr_densify_stats(const int32_t* radii, const float* dmeans2D, int32_t P, float* max_radii2D,
                      float* grad_accum, float* denom, void* stream);
/* ... skipped on the device when *guard_k > guard_cap (as gsr_adam_step_guarded). */
int gsr_densify_stats_guarded(const int32_t* radii, const float* dmeans2D, int32_t P, float* max_radii2D,
                              float* grad_accum, float* denom, const uint32_t* guard_k, uint32_t guard_cap,
                              void* stream);

/* MCMC densification, the per-iteration noise: for each of the P Gaussians, from the RAW leaves,
 *   s = exp(scale_raw), q = rot_raw / max(|rot_raw|, 1e-12) (w first), R = R(q), o = sigmoid(opac_raw),
 *   gate = 1 / (1 + exp(100 (o - 0.005)))       (upstream's op_sigmoid(1 - o, k = 100, x0 = 0.995))
 *   xyz += R diag(s^2) R^T (noise * gate * strength)
 * noise: P x 3 standard-normal floats the caller drew (the kernel is a pure function of its inputs);
 * strength = noise_lr * the scheduled xyz rate, finite and >= 0.  The gate reaches exactly 0 for
 * opaque Gaussians (exp overflows to +inf, 1 / (1 + inf) = 0); such a row keeps the bits of its xyz,
 * and so does every row at strength 0 (no launch).  rot_raw 16-byte aligned, the others 4.  Skipped
 * on the device when *guard_k > guard_cap (as gsr_adam_step_guarded; NULL: never skipped).  P == 0:
 * returns 0.  One launch, no scratch, no atomics; 68 B of traffic per Gaussian. */
int gsr_mcmc_noise(float* xyz, const float* scale_raw, const float* rot_raw, const float* opac_raw,
                   const float* noise, int32_t P, float strength,
                   const uint32_t* guard_k, uint32_t guard_cap, void* stream);

/* MCMC densification, the relocation: row i (ACTIVATED opacity o, scale, of n sampled rows) is about
 * to be shared by N = ratios[i] clamped to [1, GSR_MCMC_MAX_RATIO] Gaussians.  With
 *   x = 1 - (1 - o)^(1/N)
 *   D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)
 *     = sum_{k=0..N-1} C(N, k+1) (-1)^k x^(k+1) / sqrt(k+1)
 *   new_scales = (o / D) scales,  new_opacities = min(max(x, min_opacity), 1 - 2^-24).
 * x, D and o / D are evaluated in fp64 (binomials from a table inside the library) and each output
 * is rounded to fp32 once.  A row with o <= 0 keeps its scale and takes min_opacity.  min_opacity in
 * (0, 1); n == 0: returns 0.  The outputs must not overlap the inputs (not checked). */
#define GSR_MCMC_MAX_RATIO 51
int gsr_mcmc_relocate(const float* opacities, const float* scales, const int32_t* ratios, int32_t n,
                      float min_opacity, float* new_opacities, float* new_scales, void* stream);

/* Stream compaction: idx_out[0 .. count) = the i with mask[i] != 0, ascending; *count_out
 * (device int32).  scratch: gsr_compact_scratch_bytes(n). */
size_t gsr_compact_scratch_bytes(int32_t n);
int gsr_compact_index(const uint8_t* mask, int32_t n, int32_t* idx_out, int32_t* count_out, void* scratch,
                      void* stream);

typedef struct gsr_row_copy {
    const float* src;        /* rows of `width` floats */
    float* dst;              /* n_out rows of `width` floats (must not alias src) */
    int32_t width;
} gsr_row_copy;
#define GSR_GATHER_MAX 24
/* dst[i] = src[idx[i]] (row copies) for every entry of `copies` (HOST array) in one launch. */
int gsr_gather_rows(const gsr_row_copy* copies, int32_t ncopies, const int32_t* idx, int32_t n_out,
                    void* stream);

/* Point-cloud initialisation (upstream create_from_pcd, whose distCUDA2 this
 * replaces -- the reference's point-cloud branch is commented out,
 * src/scene/dataset_readers.cpp:198-219): dist2[i] = mean of the squared distances from point i
 * to its 3 nearest OTHER points (exact; with fewer than 3 other points the missing ones count as
 * FLT_MAX, as in upstream's kernel, so the mean is FLT_MAX / 3 or overflows to +inf).
 * points: N x 3 f32 device; scratch: gsr_knn_scratch_bytes(N) bytes. */
size_t gsr_knn_scratch_bytes(int32_t N);
int gsr_knn_mean_dist2(const float* points, int32_t N, float* dist2, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_GSR_TRAIN_H */
