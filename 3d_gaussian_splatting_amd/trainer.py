"""Training step around the rasterizer, on the HIP kernels of
include/gsr/gsr_train.h.

What it mirrors in the reference (seiya-kumada/3d_gaussian_splatting):

* ``OptimizationParams``      src/arguments/params.h:50-91 (same fields and defaults).
* ``GaussianTrainer.setup``   GaussianModel::setup, src/scene/gaussian_model.cpp:316-352: six
  Adam instances with default AdamOptions (betas 0.9/0.999, eps 1e-8) and the xyz LR
  schedule.  The reference passes (init, final, delay_mult, max_steps) to a five-argument
  get_expon_lr_func (gaussian_model.cpp:347-351 against general_utils.h:8-13), which binds
  delay_mult to lr_delay_steps; the build calls it with the
  arguments the names say (delay_steps = 0, delay_mult, max_steps).
* ``update_learning_rate`` / ``oneup_SH_degree`` and the per-iteration order
  src/utils/train_utils.cpp:128-145 (LR update, SH degree +1 every 1000 iterations, render,
  loss, backward, statistics, densification, optimizer step).
* the statistics tensors ``max_radii2D_ / xyz_gradient_accum_ / denom_``
  (src/scene/gaussian_model.h:18-20; (N) here, not the reference's {1}-shaped accumulator,
  gaussian_model.cpp:319, Appendix A).
* densify_and_clone / densify_and_split / prune_points / reset_opacity: the upstream 3DGS
  semantics the reference's stats tensors exist for (the reference has no densification
  code).
* ``capture`` / ``restore``: GaussianModel::capture / restore (gaussian_model.cpp:76-267);
  ``from_point_cloud`` / ``save_ply`` / ``from_ply``: the upstream create_from_pcd / save_ply /
  load_ply, the k-NN scale initialisation on the GPU.

Device work per iteration, all through the C ABI: gsr_activate -> gsr_forward -> loss
forward/backward -> gsr_backward -> gsr_densify_stats -> gsr_adam_step (one launch for the
six groups, activation backward fused; with opt.train_exposure gsr_exposure_forward /
gsr_exposure_backward around the loss and one more guarded Adam launch for the per-view exposure
tensor); with a depth target (``step(gt_depth=...)``, upstream
3DGS's depth regulariser -- the reference has none) the render is gsr_forward_aux /
gsr_backward_aux with gsr_depth_loss between them; with opt.densify_strategy = "mcmc" (gsplat's
MCMCStrategy -- neither upstream nor the reference has it) no gsr_densify_stats, gsr_mcmc_noise after
the Adam step and gsr_mcmc_relocate inside the refinements (``mcmc_refine``).  No host synchronisation inside ``step`` (the loss
stays on the device); densification (every ``densification_interval`` iterations) reads
counts back.  The forward's binning runs under a capacity bound (``BinningCapacity``), so K is
not read back either: the first render after a change in the point set is sized exactly (one
read of K), later ones by 1.5x the largest K seen, checked one iteration late from a pinned
copy.  No CPU fallback: the HIP library is required.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import native, pose, scene_io
from .general import build_rotation, get_expon_lr_func
from .rasterizer import CAbiRasterizer

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ACTS = {"xyz": native.ACT_NONE, "f_dc": native.ACT_NONE, "f_rest": native.ACT_NONE,
        "opacity": native.ACT_SIGMOID, "scaling": native.ACT_EXP, "rotation": native.ACT_NORMALIZE4}


def _f32(x: float) -> float:
    return float(np.float32(x))


@dataclass
class OptimizationParams:
    """src/arguments/params.h:50-91.  The reference's fields are C++ float: the defaults here are
    those float values (so the C++ gsr::Trainer, which keeps the reference's struct, computes
    from the same numbers)."""
    iterations: int = 30_000
    position_lr_init: float = _f32(0.00016)
    position_lr_final: float = _f32(0.0000016)
    position_lr_delay_mult: float = _f32(0.01)
    position_lr_max_steps: int = 30_000
    feature_lr: float = _f32(0.0025)
    opacity_lr: float = _f32(0.05)
    scaling_lr: float = _f32(0.005)
    rotation_lr: float = _f32(0.001)
    percent_dense: float = _f32(0.01)
    lambda_dssim: float = _f32(0.2)
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_from_iter: int = 500
    densify_until_iter: int = 15_000
    densify_grad_threshold: float = _f32(0.0002)
    random_background: bool = False
    # depth supervision (upstream 3DGS's depth regulariser; the reference's struct has none):
    # the weight decays exponentially from _init to _final over `iterations`
    depth_l1_weight_init: float = 1.0
    depth_l1_weight_final: float = 0.01
    depth_inverse: bool = True        # supervise sum w / z (upstream's invDepth)
    depth_normalized: bool = False    # pred = depth / alpha where alpha >= depth_alpha_min
    depth_alpha_min: float = 0.5      # a design default, not a tuned value
    # anti-aliased rendering (upstream's `antialiasing`; the reference's struct has none): every
    # render of step() blends the compensated opacity (gsr.h GSR_FLAG_ANTIALIAS)
    antialiasing: bool = False
    # "default": the dense Adam step; "sparse_adam" (upstream's optimizer_type; the reference's
    # struct has none): only the Gaussians the iteration's view rendered (radii > 0) are stepped
    optimizer_type: str = "default"
    # trained per-view exposure (upstream's train_test_exp / use_trained_exp; the reference's struct
    # has none): a (3, 4) affine colour transform per training image applied to the render in front
    # of the photometric loss, with an Adam and an exponential LR schedule of its own (upstream's
    # defaults).  exposure_clamp: the exposed image is clamped to [0, 1], as upstream's render is;
    # it applies on the exposure path only
    train_exposure: bool = False
    exposure_lr_init: float = 0.01
    exposure_lr_final: float = 0.001
    exposure_lr_delay_steps: int = 0
    exposure_lr_delay_mult: float = 0.0
    exposure_clamp: bool = True
    # pose refinement (gsplat's pose_opt, the BARF family; neither upstream 3DGS nor the reference has
    # it): one rigid correction per training view (pose.py), stepped by a host-side Adam per view row
    # from the rasterizer's camera gradients (gsr_backward_posed), exponential LR schedule over
    # `iterations`; the translation half's rate is multiplied by spatial_lr_scale, as the xyz rate is.
    # Design defaults, not tuned values
    train_poses: bool = False
    pose_lr_init: float = 1e-4
    pose_lr_final: float = 1e-6
    pose_lr_delay_steps: int = 0
    pose_lr_delay_mult: float = 0.0
    # "default": upstream's clone / split / prune on a gradient threshold with the opacity reset;
    # "mcmc" (gsplat's MCMCStrategy, Kheradmand et al. 2024; neither upstream 3DGS nor the reference
    # has it): dead Gaussians are relocated onto live ones, the set grows by mcmc_growth per
    # refinement up to the hard limit cap_max and then keeps that size, no opacity reset, a
    # covariance-shaped noise on the means every step (gsr_mcmc_noise, strength noise_lr x the
    # scheduled xyz rate) and two L1 regularisers, opacity_reg x mean(opacity) and scale_reg x
    # mean(scale).  noise_lr, the regularisers, mcmc_min_opacity and mcmc_growth are gsplat's defaults
    densify_strategy: str = "default"
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    mcmc_min_opacity: float = 0.005
    mcmc_growth: float = 1.05
    # importance pruning (RadSplat's post-hoc pruning; LightGaussian and Mini-Splatting rank alike;
    # neither upstream 3DGS nor the reference has it): at these iterations train_loop.train drops the
    # Gaussians whose score over all training views (GaussianTrainer.importance: "max_w", "sum_w" or
    # "hits") is below the threshold -- 0.01 on max_w is RadSplat's value.  An iteration that also
    # densifies is skipped.  Empty: nothing new runs.  Refused with densify_strategy = "mcmc", whose
    # cap-bound point set must not shrink
    importance_prune_iters: tuple = ()
    importance_prune_score: str = "max_w"
    importance_prune_threshold: float = 0.01


OPTIMIZER_TYPES = ("default", "sparse_adam")
DENSIFY_STRATEGIES = ("default", "mcmc")
IMPORTANCE_SCORES = ("max_w", "sum_w", "hits")  # rasterizer.SCORE_NAMES


class PoseState:
    """The per-view pose corrections and their Adam state, float64 on the host: delta (N, 6) =
    (omega, tau) per view (pose.py), exp_avg, exp_avg_sq, and each row's own step count."""

    def __init__(self, n_views: int):
        n = int(n_views)
        if n <= 0:
            raise ValueError("PoseState: n_views must be positive")
        self.delta = np.zeros((n, 6), np.float64)
        self.exp_avg = np.zeros((n, 6), np.float64)
        self.exp_avg_sq = np.zeros((n, 6), np.float64)
        self.steps = np.zeros(n, np.int64)

    def adam_row(self, row: int, grad, lr: float, spatial_lr_scale: float = 1.0, beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-8) -> None:
        """One torch::optim::Adam step (default options, no weight decay) of row `row` alone, at that
        row's step count; the translation half steps at lr * spatial_lr_scale."""
        g = np.asarray(grad, np.float64).reshape(6)
        self.steps[row] += 1
        t = int(self.steps[row])
        m, v = self.exp_avg[row], self.exp_avg_sq[row]
        m *= beta1
        m += (1.0 - beta1) * g
        v *= beta2
        v += (1.0 - beta2) * g * g
        rates = lr * np.array([1.0, 1.0, 1.0, spatial_lr_scale, spatial_lr_scale, spatial_lr_scale])
        denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** t) + eps
        self.delta[row] -= (rates / (1.0 - beta1 ** t)) * (m / denom)

    def state_dict(self) -> dict:
        return {k: torch.from_numpy(getattr(self, k).copy()) for k in ("delta", "exp_avg", "exp_avg_sq", "steps")}

    @classmethod
    def from_state_dict(cls, d: dict) -> "PoseState":
        st = cls(int(d["delta"].shape[0]))
        for k, dt in (("delta", np.float64), ("exp_avg", np.float64), ("exp_avg_sq", np.float64), ("steps", np.int64)):
            setattr(st, k, np.ascontiguousarray(d[k].detach().cpu().numpy(), dtype=dt).copy())
        return st


def _device(device) -> torch.device:
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class TrainKernels:
    """ctypes front-end of include/gsr/gsr_train.h with torch-owned device memory."""

    def __init__(self, device="cuda"):
        self.device = _device(device)
        self.L = native.load_hip()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {native.last_error()}")

    def _need(self, what, name, t, shape, dtype=torch.float32):
        """t must be contiguous, of `dtype`, on this device and, unless `shape` is None, of that
        shape; a str entry of `shape` ("P") stands for any size."""
        ok = t.is_contiguous() and t.dtype == dtype and t.device == self.device
        if ok and shape is not None and tuple(t.shape) != shape:
            ok = t.dim() == len(shape) and all(isinstance(s, str) or int(d) == s for d, s in zip(t.shape, shape))
        if not ok:
            txt = "" if shape is None else "(" + ", ".join(map(str, shape)) + ("," if len(shape) == 1 else "") + ") "
            raise ValueError(f"{what}: {name} must be a contiguous {'f32' if dtype == torch.float32 else 'int32'} "
                             f"{txt}tensor on {self.device}")

    def activate(self, scale_raw, rot_raw, opac_raw):
        P = int(scale_raw.shape[0])
        s = torch.empty_like(scale_raw)
        q = torch.empty_like(rot_raw)
        o = torch.empty_like(opac_raw)
        self._check(self.L.gsr_activate(_p(scale_raw), _p(rot_raw), _p(opac_raw), P, _p(s), _p(q), _p(o),
                                        _stream(self.device)), "gsr_activate")
        return s, q, o

    def loss_forward(self, img, gt, lambda_dssim):
        """-> (stats (3,) device tensor [loss, l1, ssim], maps scratch for loss_backward)."""
        C, H, W = (int(v) for v in img.shape)
        if tuple(gt.shape) != (C, H, W):
            raise ValueError("loss: image / ground-truth shape mismatch")
        nbytes = int(self.L.gsr_loss_scratch_bytes(C, H, W))
        maps = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        stats = torch.empty(3, dtype=torch.float32, device=self.device)
        self._check(self.L.gsr_loss_forward(_p(img), _p(gt), C, H, W, float(lambda_dssim), _p(maps), _p(stats),
                                            _stream(self.device)), "gsr_loss_forward")
        return stats, maps

    def loss_backward(self, img, gt, lambda_dssim, maps):
        C, H, W = (int(v) for v in img.shape)
        out = torch.empty_like(img)
        self._check(self.L.gsr_loss_backward(_p(img), _p(gt), C, H, W, float(lambda_dssim), _p(maps), _p(out),
                                             _stream(self.device)), "gsr_loss_backward")
        return out

    def depth_loss(self, depth, target, mask=None, alpha=None, weight=1.0, normalized=False, alpha_min=0.5):
        """gsr_depth_loss on (H, W) planes: weight * mean |(pred - target) * mask|, pred = depth or
        (normalized) depth / alpha where alpha >= alpha_min.  -> (stats (3,) device tensor
        [weighted loss, mean |e|, contributing pixels], dL_ddepth, dL_dalpha or None), gradients for
        dL/dloss = 1.  Planes may be any f32 views with contiguous pixels (a 1-element offset takes
        the kernel's scalar path)."""
        H, W = (int(v) for v in depth.shape)
        for name, t in dict(depth=depth, target=target, mask=mask, alpha=alpha).items():
            if t is not None:
                self._need("depth_loss", name, t, (H, W))
        if normalized and alpha is None:
            raise ValueError("depth_loss: normalized mode needs alpha")
        scratch = torch.empty(int(self.L.gsr_depth_loss_scratch_bytes(H, W)), dtype=torch.uint8, device=self.device)
        stats = torch.empty(3, dtype=torch.float32, device=self.device)
        dd = torch.empty_like(depth)
        da = torch.empty_like(alpha) if normalized else None
        self._check(self.L.gsr_depth_loss(_p(depth), _p(alpha) if normalized else None, _p(target),
                                          None if mask is None else _p(mask), H, W, float(weight),
                                          native.DEPTH_NORMALIZED if normalized else native.DEPTH_RAW,
                                          float(alpha_min), _p(scratch), _p(stats), _p(dd),
                                          None if da is None else _p(da), _stream(self.device)), "gsr_depth_loss")
        return stats, dd, da

    def _exposure_args(self, what, img, exposure, extra=None):
        if img.dim() != 3 or int(img.shape[0]) != 3:
            raise ValueError(f"{what}: img must be (3, H, W)")
        H, W = int(img.shape[1]), int(img.shape[2])
        for name, t in (("img", img), ("dL_dout", extra)):
            if t is not None:
                self._need(what, name, t, (3, H, W))
        self._need(what, "exposure", exposure, (3, 4))
        return H, W

    def exposure_forward(self, img, exposure, clamp=False):
        """gsr_exposure_forward: out_j = sum_i exposure[i][j] img_i + exposure[j][3] per pixel of a
        (3, H, W) image, clamped to [0, 1] with `clamp`.  exposure: a (3, 4) device tensor, or a
        contiguous row of the (N, 3, 4) parameter (never read by the host)."""
        H, W = self._exposure_args("exposure_forward", img, exposure)
        out = torch.empty_like(img)
        self._check(self.L.gsr_exposure_forward(_p(img), _p(exposure), H, W, native.EXPOSURE_CLAMP if clamp else 0,
                                                _p(out), _stream(self.device)), "gsr_exposure_forward")
        return out

    def exposure_backward(self, img, exposure, dL_dout, clamp=False, out=None):
        """gsr_exposure_backward -> (dL_dimg (3, H, W), dL_dexposure (3, 4)); with `clamp` the
        gradient is dropped where the unclamped value left [0, 1].  out: a contiguous (3, 4) f32
        view (a row of a larger gradient tensor) that receives dL_dexposure instead of a new one."""
        H, W = self._exposure_args("exposure_backward", img, exposure, dL_dout)
        dE = torch.empty((3, 4), dtype=torch.float32, device=self.device) if out is None else out
        self._need("exposure_backward", "out", dE, (3, 4))
        scratch = torch.empty(int(self.L.gsr_exposure_scratch_bytes(H, W)), dtype=torch.uint8, device=self.device)
        dimg = torch.empty_like(img)
        self._check(self.L.gsr_exposure_backward(_p(img), _p(exposure), _p(dL_dout), H, W,
                                                 native.EXPOSURE_CLAMP if clamp else 0, _p(scratch), _p(dimg),
                                                 _p(dE), _stream(self.device)), "gsr_exposure_backward")
        return dimg, dE

    def adam_step(self, groups, beta1=0.9, beta2=0.999, eps=1e-8, guard=None, visibility=None):
        """groups: list of dicts(param, grad, exp_avg, exp_avg_sq, act, step, lr), one launch.
        guard = (k_device, bound): the step is skipped on the device when the render's K
        exceeded the bound it ran under (gsr_adam_step_guarded).
        visibility: the rasterizer's radii, a contiguous int32 (P,) device tensor; only the rows of
        Gaussians with radii > 0 are stepped, the others keep their bytes (gsr_adam_step_sparse)."""
        if visibility is not None:
            self._need("adam", "visibility", visibility, ("P",), torch.int32)
            P = int(visibility.numel())
            for g in groups:
                n = g["param"].numel()
                if (n % P) if P else n:
                    raise ValueError(f"adam: a group of {n} elements is no multiple of P = {P}")
        arr = (native.AdamGroup * len(groups))()
        for i, g in enumerate(groups):
            for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
                t = g[k]
                self._need("adam", k, t, None)
                if t.numel() != g["param"].numel():
                    raise ValueError(f"adam: {k} size mismatch")
                setattr(arr[i], k, t.data_ptr())
            arr[i].n = g["param"].numel()
            arr[i].act = int(g["act"])
            arr[i].step = int(g["step"])
            arr[i].lr = float(g["lr"])
        gk, gcap = _guard(guard)
        if visibility is not None:
            self._check(self.L.gsr_adam_step_sparse(arr, len(groups), _p(visibility), P, float(beta1), float(beta2),
                                                    float(eps), gk, gcap, _stream(self.device)),
                        "gsr_adam_step_sparse")
            return
        self._check(self.L.gsr_adam_step_guarded(arr, len(groups), float(beta1), float(beta2), float(eps), gk, gcap,
                                                 _stream(self.device)), "gsr_adam_step")

    def densify_stats(self, radii, dmeans2D, max_radii2D, grad_accum, denom, guard=None):
        P = int(radii.shape[0])
        gk, gcap = _guard(guard)
        self._check(self.L.gsr_densify_stats_guarded(_p(radii), _p(dmeans2D), P, _p(max_radii2D), _p(grad_accum),
                                                     _p(denom), gk, gcap, _stream(self.device)), "gsr_densify_stats")

    def mcmc_noise(self, xyz, scale_raw, rot_raw, opac_raw, noise, strength, guard=None):
        """gsr_mcmc_noise, in place on xyz (P, 3): xyz += R diag(s^2) R^T (noise * gate * strength) from
        the raw leaves scale_raw (P, 3), rot_raw (P, 4), opac_raw (P, 1) or (P,), with noise (P, 3)
        standard-normal floats the caller drew.  guard as adam_step."""
        P = int(xyz.shape[0])
        self._need("mcmc_noise", "xyz", xyz, (P, 3))
        self._need("mcmc_noise", "scale_raw", scale_raw, (P, 3))
        self._need("mcmc_noise", "rot_raw", rot_raw, (P, 4))
        self._need("mcmc_noise", "opac_raw", opac_raw, (P, 1) if opac_raw.dim() == 2 else (P,))
        self._need("mcmc_noise", "noise", noise, (P, 3))
        gk, gcap = _guard(guard)
        self._check(self.L.gsr_mcmc_noise(_p(xyz), _p(scale_raw), _p(rot_raw), _p(opac_raw), _p(noise), P,
                                          float(strength), gk, gcap, _stream(self.device)), "gsr_mcmc_noise")

    def mcmc_relocate(self, opacities, scales, ratios, min_opacity):
        """gsr_mcmc_relocate on n sampled rows: activated opacities (n,), scales (n, 3) and int32
        ratios (n,) (how many Gaussians share the row, clamped to [1, native.MCMC_MAX_RATIO]) ->
        (new_opacities (n,), new_scales (n, 3))."""
        n = int(opacities.shape[0])
        self._need("mcmc_relocate", "opacities", opacities, (n,))
        self._need("mcmc_relocate", "scales", scales, (n, 3))
        self._need("mcmc_relocate", "ratios", ratios, (n,), torch.int32)
        new_o, new_s = torch.empty_like(opacities), torch.empty_like(scales)
        self._check(self.L.gsr_mcmc_relocate(_p(opacities), _p(scales), _p(ratios), n, float(min_opacity), _p(new_o),
                                             _p(new_s), _stream(self.device)), "gsr_mcmc_relocate")
        return new_o, new_s

    def compact_index(self, mask: torch.Tensor) -> torch.Tensor:
        """Ascending int32 indices of the nonzero entries of a bool / uint8 mask (one D2H read)."""
        m = mask.to(torch.uint8).contiguous()
        n = int(m.numel())
        idx = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(1, dtype=torch.int32, device=self.device)
        scratch = torch.empty(int(self.L.gsr_compact_scratch_bytes(n)), dtype=torch.uint8, device=self.device)
        self._check(self.L.gsr_compact_index(_p(m), n, _p(idx), _p(cnt), _p(scratch), _stream(self.device)),
                    "gsr_compact_index")
        return idx[: int(cnt.item())]

    def knn_mean_dist2(self, points: torch.Tensor) -> torch.Tensor:
        """Mean squared distance of each point to its 3 nearest others (exact; gsr_knn_mean_dist2)."""
        self._need("knn", "points", points, ("N", 3))
        n = int(points.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        scratch = torch.empty(int(self.L.gsr_knn_scratch_bytes(n)), dtype=torch.uint8, device=self.device)
        self._check(self.L.gsr_knn_mean_dist2(_p(points), n, _p(out), _p(scratch), _stream(self.device)),
                    "gsr_knn_mean_dist2")
        return out

    def gather_rows(self, tensors, idx: torch.Tensor):
        """[t[idx] for t in tensors] (rows) in one launch; tensors are (N, ...) f32."""
        n_out = int(idx.numel())
        outs = [torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=self.device)
                for t in tensors]
        if n_out == 0 or not tensors:
            return outs
        live = [i for i, t in enumerate(tensors) if math.prod(t.shape[1:]) > 0]  # skip (N, 0, 3) rows
        idx32 = idx.to(torch.int32).contiguous()
        for i0 in range(0, len(live), native.GATHER_MAX):
            chunk = live[i0:i0 + native.GATHER_MAX]
            arr = (native.RowCopy * len(chunk))()
            for j, i in enumerate(chunk):
                t = tensors[i]
                if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device):
                    raise ValueError("gather_rows: contiguous f32 device tensors only")
                arr[j].src, arr[j].dst = t.data_ptr(), outs[i].data_ptr()
                arr[j].width = int(math.prod(t.shape[1:]))
            self._check(self.L.gsr_gather_rows(arr, len(chunk), _p(idx32), n_out, _stream(self.device)),
                        "gsr_gather_rows")
        return outs


def _guard(guard):
    """(device pointer of K, bound) for the *_guarded entry points; (None, 0) = no guard."""
    if guard is None:
        return None, 0
    k, cap = guard
    return ctypes.c_void_p(k.data_ptr()), int(cap)


class BinningOverflowError(OverflowError):
    """A bounded render's K exceeded its bound (strict BinningCapacity): that render dropped
    instances, and the iteration that used it has been applied."""


class BinningCapacity:
    """max_rendered for the trainer's renders without a per-iteration host read of K.

    0 (exact sizing, the forward reads K back) right after the point set changes; afterwards
    ``headroom`` x the largest K seen, rounded up.  Each bounded render's K (the scan's device
    counter) is copied to a pinned slot and checked once its event has completed -- one or two
    iterations later, never waiting.  K above the bound at that check means that render was
    truncated (its kernels clamp to the bound; GSR_ERR_OVERFLOW semantics) and the iteration
    that used it has already run: its densification statistics and Adam step were skipped ON
    THE DEVICE (the trainer passes the render's K and bound to the *_guarded kernels, so a
    truncated render never updates the model), it is counted in ``overflows`` (with a warning
    the first time), the next render is sized exactly again, and with ``strict=True`` a
    BinningOverflowError is raised at that check instead.  The bound covers the largest K of
    the views rendered since the last point-set change with 1.5x + 64k headroom; views are
    re-rendered every len(views) iterations, so a view larger than that bound can only be one
    not yet seen since the change (the 30k-iteration loop: 0 overflows)."""

    def __init__(self, device, headroom: float = 1.5, ring: int = 8, strict: bool = False):
        self.headroom = float(headroom)
        self.strict = bool(strict)
        self.cap = 0
        self.k_max = 0
        self.overflows = 0
        self.exact_reads = 0
        pin = torch.cuda.is_available()
        self.slots = [torch.zeros(1, dtype=torch.int32, pin_memory=pin) for _ in range(ring)]
        self.pending: list = []  # (slot, event, cap)
        self.next_slot = 0

    def bound(self) -> int:
        self.poll()
        return self.cap

    def _grow(self):
        self.cap = (int(self.k_max * self.headroom) + 65536 + 4095) // 4096 * 4096

    def reset(self):
        """The point set changed: the next render is sized exactly."""
        self.pending.clear()
        self.cap = 0
        self.k_max = 0

    def observe(self, st):
        """After a forward: record its K (exact read, or an async copy under a bound)."""
        if self.cap == 0:
            self.exact_reads += 1
            self.k_max = max(self.k_max, st.num_rendered)
            self._grow()
            return
        if len(self.pending) == len(self.slots):
            self.pending[0][1].synchronize()
            self.poll()
        slot = self.slots[self.next_slot]
        self.next_slot = (self.next_slot + 1) % len(self.slots)
        slot.copy_(st.k_device(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(st.color.device))
        self.pending.append((slot, ev, self.cap))

    def poll(self):
        while self.pending and self.pending[0][1].query():
            slot, _, cap = self.pending.pop(0)
            k = int(slot.item())
            if k > cap:
                if self.overflows == 0:
                    warnings.warn(f"BinningCapacity: a render's K = {k} exceeded its bound {cap}; that iteration's "
                                  "update was skipped on the device and renders are sized exactly again",
                                  RuntimeWarning, stacklevel=2)
                self.overflows += 1
                self.k_max = max(self.k_max, k)
                self.pending.clear()
                self.cap = 0  # the next render is sized exactly
                if self.strict:
                    raise BinningOverflowError(f"a render's K = {k} exceeded its bound {cap}")
                return
            if k > self.k_max:
                self.k_max = k
                if k * 1.2 > self.cap:
                    self._grow()


class GaussianTrainer:
    """The reference GaussianModel's training state (raw leaves, Adam moments, statistics)
    with the per-iteration step on the HIP kernels."""

    def __init__(self, xyz, f_dc, f_rest, opacity, scaling, rotation, max_sh_degree: int,
                 opt: OptimizationParams | None = None, spatial_lr_scale: float = 1.0, device="cuda",
                 seed: int = 0, cameras_extent: float | None = None):
        self.device = _device(device)
        dev = self.device
        f = lambda a, shape: torch.as_tensor(a, dtype=torch.float32).reshape(shape).to(dev).contiguous()
        P = int(torch.as_tensor(xyz).shape[0])
        self.params = {"xyz": f(xyz, (P, 3)), "f_dc": f(f_dc, (P, 1, 3)),
                       "f_rest": f(f_rest, (P, -1, 3)), "opacity": f(opacity, (P, 1)),
                       "scaling": f(scaling, (P, 3)), "rotation": f(rotation, (P, 4))}
        self.max_sh_degree = int(max_sh_degree)
        self.active_sh_degree = 0
        self._guard = None  # (K device counter, bound) of the last bounded render
        # the reference's CoreParams::spatial_lr_scale_ is a float (gaussian_model.h): held at
        # f32 precision, so a capture / restore round trip (which stores it as float) is exact
        self.spatial_lr_scale = _f32(spatial_lr_scale)
        # scene extent for the clone / split threshold and the world-size prune; upstream sets
        # spatial_lr_scale to this same value (the nerf++ radius of the training cameras)
        self.cameras_extent = float(spatial_lr_scale if cameras_extent is None else cameras_extent)
        self.k = TrainKernels(dev)
        self.rast = CAbiRasterizer(dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.binning = BinningCapacity(dev)
        self.exposure = None  # (N, 3, 4) after setup_exposure
        self.exposure_names = None
        self.poses = None  # PoseState after setup_poses
        self._pose_pending = {}
        self.pose_updates_dropped = 0
        self.setup(opt or OptimizationParams())

    @classmethod
    def from_point_cloud(cls, points, colors, max_sh_degree: int, spatial_lr_scale: float,
                         opt: OptimizationParams | None = None, device="cuda", seed: int = 0) -> "GaussianTrainer":
        """Upstream create_from_pcd (the reference has none: its point-cloud branch is commented
        out, src/scene/dataset_readers.cpp:198-219): means = the points, f_dc = RGB2SH(colour),
        f_rest = 0, every scale axis = log(sqrt(max(d, 1e-7))) with d the mean squared distance to
        the 3 nearest other points (gsr_knn_mean_dist2 on the GPU), rotation = (1, 0, 0, 0),
        opacity = inverse_sigmoid(0.1); spatial_lr_scale = the cameras' extent."""
        dev = _device(device)
        pts = torch.as_tensor(np.asarray(points, np.float32), device=dev).reshape(-1, 3).contiguous()
        n = int(pts.shape[0])
        d2 = TrainKernels(dev).knn_mean_dist2(pts)
        scales = torch.log(torch.sqrt(torch.clamp_min(d2, 1e-7)))[:, None].repeat(1, 3)
        rots = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        rots[:, 0] = 1.0
        o = torch.full((n, 1), 0.1, dtype=torch.float32, device=dev)
        opac = torch.log(o / (1 - o))
        rgb = torch.as_tensor(np.asarray(colors, np.float32), device=dev).reshape(-1, 3)
        f_dc = ((rgb - 0.5) / scene_io.SH_C0)[:, None, :]
        f_rest = torch.zeros((n, (max_sh_degree + 1) ** 2 - 1, 3), dtype=torch.float32, device=dev)
        return cls(pts, f_dc, f_rest, opac, scales, rots, max_sh_degree, opt, spatial_lr_scale, dev, seed)

    # ---------------------------------------------------------------- checkpoints / PLY
    def capture(self, path: str) -> None:
        """GaussianModel::capture (src/scene/gaussian_model.cpp:76-131, 228-246): parameters,
        statistics, SH degree, spatial LR scale and every group's Adam state, one file."""
        self.flush_poses()
        scene_io.save_checkpoint(path, {
            "poses": None if self.poses is None else self.poses.state_dict(),
            "active_sh_degree": self.active_sh_degree, "spatial_lr_scale": self.spatial_lr_scale,
            "cameras_extent": self.cameras_extent, "params": self.params, "max_radii2D": self.max_radii2D, "xyz_gradient_accum": self.xyz_gradient_accum,
            "denom": self.denom, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "steps": self.steps,
            "exposure": None if self.exposure is None else {
                "param": self.exposure, "exp_avg": self.exposure_exp_avg, "exp_avg_sq": self.exposure_exp_avg_sq,
                "step": self.exposure_step, "names": self.exposure_names}})

    def restore(self, path: str, opt: OptimizationParams | None = None) -> None:
        """GaussianModel::restore (gaussian_model.cpp:248-267): setup(opt), then the captured
        tensors and Adam states replace the fresh ones."""
        st = scene_io.load_checkpoint(path, self.device)
        self.params = {k: v.contiguous() for k, v in st["params"].items()}
        self.spatial_lr_scale = st["spatial_lr_scale"]
        self.cameras_extent = st.get("cameras_extent", self.spatial_lr_scale)
        self.setup(opt or self.opt)
        self.active_sh_degree = st["active_sh_degree"]
        self.max_radii2D, self.xyz_gradient_accum, self.denom = st["max_radii2D"], st["xyz_gradient_accum"], st["denom"]
        for k in self.params:
            if k in st["exp_avg"]:
                self.exp_avg[k] = st["exp_avg"][k].contiguous()
                self.exp_avg_sq[k] = st["exp_avg_sq"][k].contiguous()
                self.steps[k] = st["steps"][k]
        ex = st.get("exposure")  # absent in a checkpoint without exposure: it stays unset
        self.exposure = self.exposure_names = None
        if ex is not None:
            self.exposure = ex["param"].contiguous()
            self.exposure_exp_avg, self.exposure_exp_avg_sq = ex["exp_avg"].contiguous(), ex["exp_avg_sq"].contiguous()
            self.exposure_step, self.exposure_names = ex["step"], ex["names"]
        ps = st.get("poses")  # absent in a checkpoint without poses: they stay unset
        self._pose_pending = {}
        self.poses = None if ps is None else PoseState.from_state_dict(ps)
        if ps is not None:
            self._pose_slots(int(self.poses.delta.shape[0]))

    def save_ply(self, path: str) -> None:
        """The raw leaves in the upstream point-cloud PLY layout (scene_io.save_gaussians_ply)."""
        scene_io.save_gaussians_ply(path, **self.params)

    @classmethod
    def from_ply(cls, path: str, max_sh_degree: int, opt: OptimizationParams | None = None,
                 spatial_lr_scale: float = 1.0, device="cuda", seed: int = 0) -> "GaussianTrainer":
        """Upstream load_ply: the leaves of a Gaussian PLY, active SH degree = max_sh_degree."""
        g = scene_io.load_gaussians_ply(path, max_sh_degree)
        tr = cls(g["xyz"], g["f_dc"], g["f_rest"], g["opacity"], g["scaling"], g["rotation"], max_sh_degree, opt,
                 spatial_lr_scale, device, seed)
        tr.active_sh_degree = max_sh_degree
        return tr

    # ---------------------------------------------------------------- GaussianModel surface
    @property
    def num_points(self) -> int:
        return int(self.params["xyz"].shape[0])

    def setup(self, opt: OptimizationParams):
        """GaussianModel::setup (gaussian_model.cpp:316-352)."""
        if opt.optimizer_type not in OPTIMIZER_TYPES:
            raise ValueError(f"optimizer_type must be one of {OPTIMIZER_TYPES}, not {opt.optimizer_type!r}")
        if opt.densify_strategy not in DENSIFY_STRATEGIES:
            raise ValueError(f"densify_strategy must be one of {DENSIFY_STRATEGIES}, not {opt.densify_strategy!r}")
        if opt.densify_strategy == "mcmc":
            for name in ("noise_lr", "opacity_reg", "scale_reg"):
                v = getattr(opt, name)
                if not (math.isfinite(v) and v >= 0.0):
                    raise ValueError(f"{name} must be a finite, non-negative number, not {v!r}")
            if not 0.0 < opt.mcmc_min_opacity < 1.0:
                raise ValueError(f"mcmc_min_opacity must lie in (0, 1), not {opt.mcmc_min_opacity!r}")
            if not (math.isfinite(opt.mcmc_growth) and opt.mcmc_growth >= 1.0):
                raise ValueError(f"mcmc_growth must be a finite number >= 1, not {opt.mcmc_growth!r}")
            if int(opt.cap_max) < 1:
                raise ValueError(f"cap_max must be positive, not {opt.cap_max!r}")
        if opt.importance_prune_score not in IMPORTANCE_SCORES:
            raise ValueError(f"importance_prune_score must be one of {IMPORTANCE_SCORES}, not "
                             f"{opt.importance_prune_score!r}")
        if not (math.isfinite(opt.importance_prune_threshold) and opt.importance_prune_threshold >= 0.0):
            raise ValueError("importance_prune_threshold must be a finite, non-negative number, not "
                             f"{opt.importance_prune_threshold!r}")
        if any(int(i) != i or i < 1 for i in opt.importance_prune_iters):
            raise ValueError(f"importance_prune_iters must be positive iteration numbers, not "
                             f"{opt.importance_prune_iters!r}")
        if opt.densify_strategy == "mcmc" and len(opt.importance_prune_iters):
            raise ValueError("importance_prune_iters cannot be combined with densify_strategy = \"mcmc\": its "
                             "point set is held at cap_max and must not shrink")
        for name in ("pose_lr_init", "pose_lr_final", "pose_lr_delay_mult"):
            v = getattr(opt, name)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be a finite, non-negative number, not {v!r}")
        if (opt.pose_lr_init == 0.0) != (opt.pose_lr_final == 0.0):
            raise ValueError("pose_lr_init and pose_lr_final must both be positive or both be 0 (frozen poses): "
                             "the schedule interpolates their logarithms")
        if int(opt.pose_lr_delay_steps) < 0:
            raise ValueError(f"pose_lr_delay_steps must be >= 0, not {opt.pose_lr_delay_steps!r}")
        self.opt = opt
        self.percent_dense = opt.percent_dense
        P = self.num_points
        z = lambda: torch.zeros(P, dtype=torch.float32, device=self.device)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = z(), z(), z()
        self.exp_avg = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.exp_avg_sq = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self.steps = {k: 0 for k in GROUPS}
        self.lr = {"xyz": opt.position_lr_init * self.spatial_lr_scale, "f_dc": opt.feature_lr,
                   "f_rest": opt.feature_lr / 20.0, "opacity": opt.opacity_lr, "scaling": opt.scaling_lr,
                   "rotation": opt.rotation_lr}
        self.xyz_scheduler = get_expon_lr_func(opt.position_lr_init * self.spatial_lr_scale,
                                               opt.position_lr_final * self.spatial_lr_scale,
                                               lr_delay_steps=0, lr_delay_mult=opt.position_lr_delay_mult,
                                               max_steps=opt.position_lr_max_steps)
        # upstream: depth_l1_weight = get_expon_lr_func(init, final, max_steps=opt.iterations)
        self.depth_weight_scheduler = get_expon_lr_func(opt.depth_l1_weight_init, opt.depth_l1_weight_final,
                                                        max_steps=opt.iterations)
        # upstream: exposure_scheduler_args = get_expon_lr_func(exposure_lr_init, exposure_lr_final,
        # lr_delay_steps, lr_delay_mult, max_steps = iterations)
        self.exposure_scheduler = get_expon_lr_func(opt.exposure_lr_init, opt.exposure_lr_final,
                                                    lr_delay_steps=opt.exposure_lr_delay_steps,
                                                    lr_delay_mult=opt.exposure_lr_delay_mult,
                                                    max_steps=opt.iterations)
        self.exposure_lr = opt.exposure_lr_init
        self.pose_scheduler = get_expon_lr_func(opt.pose_lr_init, opt.pose_lr_final,
                                                lr_delay_steps=opt.pose_lr_delay_steps,
                                                lr_delay_mult=opt.pose_lr_delay_mult, max_steps=opt.iterations)
        self.pose_lr = opt.pose_lr_init

    def setup_exposure(self, n_views: int, names=None):
        """Upstream's per-image exposure parameter: (N, 3, 4), every row eye(3, 4), with zero Adam
        moments and a step count of 0.  names (one per view) are kept for exposure.json."""
        n_views = int(n_views)
        if n_views <= 0:
            raise ValueError("setup_exposure: n_views must be positive")
        if names is not None and len(names) != n_views:
            raise ValueError("setup_exposure: one name per view")
        eye = torch.eye(3, 4, dtype=torch.float32, device=self.device)
        self.exposure = eye[None].repeat(n_views, 1, 1).contiguous()
        self.exposure_exp_avg = torch.zeros_like(self.exposure)
        self.exposure_exp_avg_sq = torch.zeros_like(self.exposure)
        self.exposure_step = 0
        self.exposure_names = None if names is None else [str(n) for n in names]

    # ---------------------------------------------------------------- pose refinement
    def _pose_slots(self, n: int):
        pin = torch.cuda.is_available()
        self._pose_grad_slots = torch.zeros((n, native.CAMERA_GRAD_FLOATS), dtype=torch.float32, pin_memory=pin)
        self._pose_k_slots = torch.zeros(n, dtype=torch.int32, pin_memory=pin)

    def setup_poses(self, n_views: int):
        """One pose correction per training view (PoseState: (N, 6) float64 deltas, all zero, with zero
        Adam moments and step counts), kept on the host, and one pinned slot per view for the camera
        gradient its next update is made from."""
        self.poses = PoseState(n_views)
        self._pose_pending = {}
        self._pose_slots(int(n_views))

    def _apply_pose(self, view: int) -> None:
        """The update view `view`'s last step left pending, if any: wait for its copy, chain the 36
        camera floats to the row's delta (pose.chain at the delta that was rendered) and take the
        row's Adam step -- unless that render's K exceeded its bound (the *_guarded kernels' rule: the
        truncated render updates nothing)."""
        pend = self._pose_pending.pop(view, None)
        if pend is None:
            return
        ev, cam, lr, bound = pend
        ev.synchronize()
        if bound > 0 and int(self._pose_k_slots[view]) > bound:
            self.pose_updates_dropped += 1
            return
        g = pose.chain(cam, torch.from_numpy(self.poses.delta[view].copy()), self._pose_grad_slots[view].clone())
        if not bool(torch.isfinite(g).all()):  # a non-finite gradient would poison the row for good
            self.pose_updates_dropped += 1
            return
        self.poses.adam_row(view, g.numpy(), lr, self.spatial_lr_scale)

    def flush_poses(self) -> None:
        """Apply every pending pose update, in view order (waits for their copies)."""
        for view in sorted(self._pose_pending):
            self._apply_pose(view)

    def refined_cameras(self, cams) -> list:
        """cams[i] corrected by view i's delta (pose.compose), after flush_poses()."""
        if self.poses is None:
            raise ValueError("refined_cameras: setup_poses was never called")
        if len(cams) != int(self.poses.delta.shape[0]):
            raise ValueError("refined_cameras: one camera per pose row")
        self.flush_poses()
        return [pose.compose(c, self.poses.delta[i]) for i, c in enumerate(cams)]

    def save_exposures(self, path: str) -> None:
        """exposure.json in upstream's layout (scene_io.save_exposures); unnamed views are "0", "1", ..."""
        if self.exposure is None:
            raise ValueError("save_exposures: setup_exposure was never called")
        names = self.exposure_names or [str(i) for i in range(int(self.exposure.shape[0]))]
        scene_io.save_exposures(path, names, self.exposure)

    def update_learning_rate(self, iteration: int) -> float:
        lr = self.xyz_scheduler(iteration)
        self.lr["xyz"] = lr
        self.exposure_lr = self.exposure_scheduler(iteration)
        self.pose_lr = self.pose_scheduler(iteration)
        return lr

    def oneup_SH_degree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---------------------------------------------------------------- one iteration
    def _forward(self, cam, bg, bound: int, aux: bool = False):
        """A forward of the current parameters under the binning bound `bound` (0: sized exactly)."""
        s, q, o = self.k.activate(self.params["scaling"], self.params["rotation"], self.params["opacity"])
        p = self.params
        kw = dict(scales=s, rotations=q, sh_dc=p["f_dc"], sh_rest=p["f_rest"] if p["f_rest"].shape[1] else None,
                  sh_degree=self.active_sh_degree, bg=bg, max_rendered=bound, antialiasing=self.opt.antialiasing)
        if aux:
            return self.rast.forward_aux(cam, p["xyz"], o.reshape(-1), inverse_depth=self.opt.depth_inverse, **kw)
        return self.rast.forward(cam, p["xyz"], o.reshape(-1), **kw)

    def render(self, cam, bg=(0.0, 0.0, 0.0), aux: bool = False):
        """The bounded forward of one iteration; aux: gsr_forward_aux (depth and alpha planes too,
        inverse depth per opt.depth_inverse) under the same bound and device guard."""
        bound = self.binning.bound()
        st = self._forward(cam, bg, bound, aux)
        # device-side guard of this iteration's statistics / Adam step (see BinningCapacity)
        self._guard = (st.k_device(), bound) if bound > 0 else None
        self.binning.observe(st)
        return st

    def step(self, iteration: int, cam, gt_image: torch.Tensor, bg=(0.0, 0.0, 0.0), densify: bool = True,
             gt_depth: torch.Tensor | None = None, depth_mask: torch.Tensor | None = None,
             view_index: int | None = None) -> dict:
        """One training iteration in the upstream order (train_utils.cpp:128-145 plus the body
        its stub omits): LR update, SH degree, render, loss, backward, densification statistics,
        densify / prune and opacity reset, then the optimizer step.  As upstream, a group whose
        tensor densification or the opacity reset has just replaced takes no Adam update in
        that iteration (torch Adam skips a fresh parameter, whose .grad is None): a densify
        iteration updates no group, an opacity reset alone skips the opacity group.  Returns
        device tensors (loss stats [loss, l1, ssim], radii); no host synchronisation unless a
        densification is due.

        gt_depth (H, W), with an optional depth_mask (H, W), adds upstream's depth term
        depth_l1_weight(iteration) * mean |(pred - gt_depth) * depth_mask| (gsr_depth_loss): the
        render is then forward_aux / backward_aux, pred the blended inverse depth (opt.depth_inverse;
        divided by alpha with opt.depth_normalized), and the dict gains "depth_stats" ([weighted
        loss, mean |e|, contributing pixels], device), "depth", "alpha" and "dL_ddepth".  Without a
        target, or at a scheduled weight of 0, the iteration is the colour-only one, call for call.

        With opt.train_exposure, view_index names the row of the (N, 3, 4) exposure parameter
        (setup_exposure) that belongs to this image: the loss sees gsr_exposure_forward of the render
        (clamped with opt.exposure_clamp), gsr_exposure_backward turns its gradient into the
        rasterizer's dL/dimage and the row's gradient, and the WHOLE exposure tensor takes one Adam
        step with a gradient that is zero outside that row (upstream's exposure_optimizer: the other
        rows keep moving on their decaying moments).  The dict gains "exposed" (the image the loss
        saw) and "dL_dexposure" (3, 4); "image" stays the raw render.  Without it the iteration is
        unchanged, call for call.

        With opt.train_poses, view_index names the row of the pose corrections (setup_poses) that
        belongs to this image, and `cam` is that view's camera as given (uncorrected): the render uses
        pose.compose(cam, delta[view_index]), the backward is gsr_backward_posed, and its 36 camera
        floats and the render's K go to the view's pinned slot by an asynchronous copy with an event.
        The row's Adam step is taken from them exactly when this view is next used (waiting on the event
        if the copy has not landed) or at flush_poses() -- never opportunistically, so step() still has
        no host synchronisation in steady state and a run does not depend on timing.  An update whose
        render overflowed its binning bound is dropped.  The dict gains "camera" (the corrected camera)
        and "dL_dcamera" (36 floats, device).  Without it the iteration is unchanged, call for call.

        With opt.densify_strategy = "mcmc" (gsplat's MCMCStrategy) the iteration keeps no densification
        statistics and never prunes or resets opacities.  The two L1 regularisers enter as constants on
        the rasterizer's gradients with respect to the ACTIVATED values: opacity_reg / P on every
        dL/dopacity and scale_reg / (3 P) on every dL/dscale (regularizer_values() gives the terms
        themselves).  When densify_from_iter < iteration < densify_until_iter and iteration %
        densification_interval == 0 (and densify), mcmc_refine() runs in front of the optimizer step;
        it changes which Gaussian a row holds, so that iteration steps no group and the binning bound
        is reset, as on a densify iteration of the default strategy.  After the optimizer step
        gsr_mcmc_noise moves the means by noise drawn from the trainer's generator, at strength
        noise_lr x the scheduled xyz rate, under the same device guard -- on refine iterations too."""
        opt = self.opt
        mcmc = opt.densify_strategy == "mcmc"
        posed = opt.train_poses
        if posed:
            if self.poses is None:
                raise ValueError("step: train_poses needs setup_poses(n_views) first")
            if view_index is None:
                raise ValueError("step: train_poses needs the view_index of this image's pose row")
            view_index = int(view_index)
            if not 0 <= view_index < int(self.poses.delta.shape[0]):
                raise ValueError(f"step: view_index {view_index} is outside the {int(self.poses.delta.shape[0])} "
                                 "pose rows")
            self._apply_pose(view_index)
            base_cam, cam = cam, pose.compose(cam, self.poses.delta[view_index])
        exposed = opt.train_exposure
        if exposed:
            if self.exposure is None:
                raise ValueError("step: train_exposure needs setup_exposure(n_views) first")
            if view_index is None:
                raise ValueError("step: train_exposure needs the view_index of this image's exposure row")
            view_index = int(view_index)
            if not 0 <= view_index < int(self.exposure.shape[0]):
                raise ValueError(f"step: view_index {view_index} is outside the {int(self.exposure.shape[0])} "
                                 "exposure rows")
        self.update_learning_rate(iteration)
        if iteration % 1000 == 0:
            self.oneup_SH_degree()
        depth_weight = self.depth_weight_scheduler(iteration) if gt_depth is not None else 0.0
        supervised = depth_weight > 0.0
        st = self.render(cam, bg, aux=supervised)
        if exposed:
            E = self.exposure[view_index]
            image = self.k.exposure_forward(st.color, E, clamp=opt.exposure_clamp)
            stats, maps = self.k.loss_forward(image, gt_image, opt.lambda_dssim)
            dexposed = self.k.loss_backward(image, gt_image, opt.lambda_dssim, maps)
            exposure_grad = torch.zeros_like(self.exposure)  # zero outside this view's row
            dimg, dE = self.k.exposure_backward(st.color, E, dexposed, clamp=opt.exposure_clamp,
                                                out=exposure_grad[view_index])
        else:
            stats, maps = self.k.loss_forward(st.color, gt_image, opt.lambda_dssim)
            dimg = self.k.loss_backward(st.color, gt_image, opt.lambda_dssim, maps)
        if supervised:
            depth_stats, dd, da = self.k.depth_loss(st.depth, gt_depth, mask=depth_mask, alpha=st.alpha,
                                                    weight=depth_weight, normalized=opt.depth_normalized,
                                                    alpha_min=opt.depth_alpha_min)
            g = self.rast.backward_aux(st, dimg, dd, da, camera_grad=True) if posed else \
                self.rast.backward_aux(st, dimg, dd, da)
        else:
            g = self.rast.backward(st, dimg, camera_grad=True) if posed else self.rast.backward(st, dimg)
        if posed and iteration < opt.iterations:
            bound = self._guard[1] if self._guard is not None else 0
            self._pose_grad_slots[view_index].copy_(g["camera"], non_blocking=True)
            if bound > 0:
                self._pose_k_slots[view_index:view_index + 1].copy_(self._guard[0], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._pose_pending[view_index] = (ev, base_cam, self.pose_lr, bound)
        grads = {"xyz": g["means3D"], "f_dc": g["sh_dc"], "opacity": g["opacities"], "scaling": g["scales"],
                 "rotation": g["rotations"]}
        if self.params["f_rest"].shape[1]:
            grads["f_rest"] = g["sh_rest"]
        replaced = set()
        if mcmc:
            P = self.num_points
            if opt.opacity_reg:
                grads["opacity"].add_(opt.opacity_reg / P)
            if opt.scale_reg:
                grads["scaling"].add_(opt.scale_reg / (3 * P))
            if (densify and opt.densify_from_iter < iteration < opt.densify_until_iter
                    and iteration % opt.densification_interval == 0):
                self.mcmc_refine()
                self.binning.reset()
                replaced.update(GROUPS)
        elif iteration < opt.densify_until_iter:
            self.k.densify_stats(st.radii, g["means2D"], self.max_radii2D, self.xyz_gradient_accum, self.denom,
                                 guard=self._guard)
            if densify:
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                    self.densify_and_prune(opt.densify_grad_threshold, 0.005, self.cameras_extent, size_threshold)
                    self.binning.reset()
                    replaced.update(GROUPS)
                if iteration % opt.opacity_reset_interval == 0:
                    self.reset_opacity()
                    self.binning.reset()
                    replaced.add("opacity")
        if iteration < opt.iterations:
            self.optimizer_step({k: v for k, v in grads.items() if k not in replaced},
                                visibility=st.radii if opt.optimizer_type == "sparse_adam" else None)
            if exposed:  # never replaced by densification: stepped on densify iterations too
                self.exposure_step += 1
                self.k.adam_step([dict(param=self.exposure, grad=exposure_grad, exp_avg=self.exposure_exp_avg,
                                       exp_avg_sq=self.exposure_exp_avg_sq, act=native.ACT_NONE,
                                       step=self.exposure_step, lr=self.exposure_lr)], guard=self._guard)
            if mcmc:
                p = self.params
                noise = torch.randn((self.num_points, 3), dtype=torch.float32, device=self.device, generator=self.gen)
                self.k.mcmc_noise(p["xyz"], p["scaling"], p["rotation"], p["opacity"], noise,
                                  opt.noise_lr * self.lr["xyz"], guard=self._guard)
        out ={"stats": stats, "radii": st.radii, "state": st, "image": st.color, "num_points": self.num_points}
        if supervised:
            out.update(depth_stats=depth_stats, depth=st.depth, alpha=st.alpha, dL_ddepth=dd)
        if exposed:
            out.update(exposed=image, dL_dexposure=dE)
        if posed:
            out.update(camera=cam, dL_dcamera=g["camera"])
        return out

    def optimizer_step(self, grads: dict, visibility: torch.Tensor | None = None):
        """One Adam step of the groups that have a gradient; visibility (the iteration's radii):
        only the rendered Gaussians' rows are stepped (optimizer_type "sparse_adam")."""
        groups = []
        for k in GROUPS:
            if k not in grads:
                continue
            self.steps[k] += 1
            groups.append(dict(param=self.params[k], grad=grads[k].reshape(self.params[k].shape).contiguous(),
                               exp_avg=self.exp_avg[k], exp_avg_sq=self.exp_avg_sq[k], act=ACTS[k],
                               step=self.steps[k], lr=self.lr[k]))
        if groups and visibility is not None:
            self.k.adam_step(groups, guard=self._guard, visibility=visibility)
        elif groups:
            self.k.adam_step(groups, guard=self._guard)

    # ---------------------------------------------------------------- densification (MCMC)
    def regularizer_values(self) -> dict:
        """The two regularisation terms of the "mcmc" strategy at the current parameters, as upstream
        writes them: opacity_reg * mean(sigmoid(opacity)) and scale_reg * mean(exp(scaling)).  step()
        applies their gradients only; this reads the values back (one host synchronisation)."""
        o = torch.sigmoid(self.params["opacity"]).mean()
        s = torch.exp(self.params["scaling"]).mean()
        return {"opacity_reg": self.opt.opacity_reg * float(o), "scale_reg": self.opt.scale_reg * float(s)}

    def _mcmc_sample(self, probs: torch.Tensor, n: int) -> torch.Tensor:
        """n indices drawn with probability proportional to probs (>= 0), with replacement, by inverse
        CDF in float64 from the trainer's generator.  (torch.multinomial stops at 2^24 categories.)
        A row of probability 0 repeats its predecessor's CDF value and is never the first above u."""
        cdf = torch.cumsum(probs.to(torch.float64), 0)
        u = torch.rand(n, dtype=torch.float64, device=self.device, generator=self.gen) * cdf[-1]
        return torch.searchsorted(cdf, u, right=True).clamp_(max=int(probs.numel()) - 1)

    def _mcmc_relocate_sources(self, src: torch.Tensor):
        """The rows `src` (int64, repeats allowed) are each about to be shared with one more Gaussian
        per occurrence: gsr_mcmc_relocate on their activated opacity and scales, written back in raw
        form (logit, log) in place, and both Adam moments of those rows zeroed in all six groups."""
        p = self.params
        counts = torch.bincount(src, minlength=self.num_points)
        ratios = (counts[src] + 1).to(torch.int32).contiguous()
        o = torch.sigmoid(p["opacity"][src, 0]).contiguous()
        s = torch.exp(p["scaling"][src]).contiguous()
        new_o, new_s = self.k.mcmc_relocate(o, s, ratios, self.opt.mcmc_min_opacity)
        # repeated sources carry equal values (same row, same ratio): the scatter's order is immaterial
        p["opacity"][src, 0] = torch.log(new_o / (1 - new_o))  # inverse_sigmoid; new_o <= 1 - 2^-24
        p["scaling"][src] = torch.log(new_s)
        for k in GROUPS:
            self.exp_avg[k][src] = 0.0
            self.exp_avg_sq[k][src] = 0.0

    def mcmc_refine(self) -> dict:
        """One refinement of the "mcmc" strategy (gsplat's MCMCStrategy._relocate_gs then _add_new_gs).

        1. dead = sigmoid(opacity) <= mcmc_min_opacity.  With dead and live rows both present: as many
           sources as dead rows are sampled from the live rows with probability proportional to their
           opacity (with replacement), the sources take the relocated opacity / scales (zeroed moments),
           and every dead row becomes a copy of its source's six parameters, in place.  The dead rows
           keep their moments, as upstream.
        2. n_new = max(0, min(cap_max, int(mcmc_growth * P)) - P) sources are sampled from all rows
           in the same way and relocated, and their copies are appended with zero moments.
        Once P == cap_max step 2 does nothing and no parameter or moment tensor is replaced again.
        Returns {"relocated": n_dead or 0, "added": n_new}; reads counts back (host synchronisation)."""
        opt = self.opt
        p = self.params
        P = self.num_points
        o = torch.sigmoid(p["opacity"][:, 0])
        dead = o <= opt.mcmc_min_opacity
        dead_idx = torch.nonzero(dead)[:, 0]
        n_dead = int(dead_idx.numel())
        relocated = 0
        if 0 < n_dead < P:
            live_idx = torch.nonzero(~dead)[:, 0]
            src = live_idx[self._mcmc_sample(o[live_idx], n_dead)]
            self._mcmc_relocate_sources(src)
            for k in GROUPS:
                p[k][dead_idx] = p[k][src]
            relocated = n_dead
        n_new = max(0, min(int(opt.cap_max), int(opt.mcmc_growth * P)) - P)
        if n_new > 0:
            src = self._mcmc_sample(torch.sigmoid(p["opacity"][:, 0]), n_new)
            self._mcmc_relocate_sources(src)
            self._append({k: p[k][src] for k in GROUPS})
        return {"relocated": relocated, "added": n_new}

    # ---------------------------------------------------------------- densification (upstream)
    def _append(self, new: dict):
        """densification_postfix: append rows (zero Adam moments), reset the statistics."""
        for k in GROUPS:
            self.params[k] = torch.cat([self.params[k], new[k].contiguous()], 0).contiguous()
            zeros = torch.zeros_like(new[k])
            self.exp_avg[k] = torch.cat([self.exp_avg[k], zeros], 0).contiguous()
            self.exp_avg_sq[k] = torch.cat([self.exp_avg_sq[k], zeros], 0).contiguous()
        P = self.num_points
        z = lambda: torch.zeros(P, dtype=torch.float32, device=self.device)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = z(), z(), z()

    def prune_points(self, mask: torch.Tensor):
        """Keep the rows where mask is False: one compaction + one multi-tensor gather of the
        parameters, both Adam moments and the three statistics."""
        idx = self.k.compact_index(~mask)
        names = [("p", k) for k in GROUPS] + [("m", k) for k in GROUPS] + [("v", k) for k in GROUPS]
        src = [{"p": self.params, "m": self.exp_avg, "v": self.exp_avg_sq}[a][k] for a, k in names]
        src += [self.xyz_gradient_accum, self.denom, self.max_radii2D]
        out = self.k.gather_rows(src, idx)
        for (a, k), t in zip(names, out):
            {"p": self.params, "m": self.exp_avg, "v": self.exp_avg_sq}[a][k] = t
        self.xyz_gradient_accum, self.denom, self.max_radii2D = out[-3], out[-2], out[-1]

    # ---------------------------------------------------------------- importance pruning
    def importance(self, cams, bg=(0.0, 0.0, 0.0)) -> dict:
        """The Gaussians' scores over `cams`, as the trainer renders them (active SH degree,
        opt.antialiasing): {"max_w", "sum_w" (float32 (P,)), "hits" (int32 (P,))}, accumulated in camera
        order by gsr_forward_scores.  Each view is rendered with exact sizing (one host read of K per
        view, no overflow: the scores are complete) and leaves the step's binning bound and device
        guard alone.  With opt.train_poses pass refined_cameras(cams)."""
        cams = list(cams)
        if not cams:
            raise ValueError("importance: no cameras")
        out = None
        for cam in cams:
            out = self.rast.scores(self._forward(cam, bg, 0), into=out)
        return out

    @staticmethod
    def _check_prune_args(score, threshold, keep_ratio):
        if score not in IMPORTANCE_SCORES:
            raise ValueError(f"prune_by_importance: score must be one of {IMPORTANCE_SCORES}, not {score!r}")
        if (threshold is None) == (keep_ratio is None):
            raise ValueError("prune_by_importance: give exactly one of threshold and keep_ratio")
        if threshold is not None and not (math.isfinite(threshold) and threshold >= 0.0):
            raise ValueError(f"prune_by_importance: threshold must be a finite, non-negative number, not {threshold!r}")
        if keep_ratio is not None and not 0.0 < keep_ratio <= 1.0:
            raise ValueError(f"prune_by_importance: keep_ratio must lie in (0, 1], not {keep_ratio!r}")

    def prune_by_importance(self, cams, score: str = "max_w", threshold: float | None = None,
                            keep_ratio: float | None = None, bg=(0.0, 0.0, 0.0)) -> int:
        """Drop the Gaussians the views `cams` use least, by importance(cams)[score]: with `threshold`
        those whose score is below it (RadSplat: max_w < 0.01); with `keep_ratio` all but the
        ceil(keep_ratio P) highest-scoring ones, ties broken by index (the lower index stays).  Exactly
        one of the two.  The rows go through prune_points, so the Adam moments and the densification
        statistics stay aligned, and the next render is sized exactly.  Refused under
        densify_strategy = "mcmc" (the point set is held at cap_max).  Returns the number removed."""
        self._check_prune_args(score, threshold, keep_ratio)
        if self.opt.densify_strategy == "mcmc":
            raise ValueError("prune_by_importance: densify_strategy = \"mcmc\" holds the point set at cap_max; "
                             "it must not shrink")
        s = self.importance(cams, bg)[score]
        P = self.num_points
        if threshold is not None:
            mask = s < threshold
        else:
            keep = min(P, math.ceil(keep_ratio * P - 1e-9))
            order = torch.sort(s, descending=True, stable=True).indices
            mask = torch.ones(P, dtype=torch.bool, device=self.device)
            mask[order[:keep]] = False
        removed = int(mask.sum().item())
        if removed:
            self.prune_points(mask)
            self.binning.reset()
        return removed

    def _rows(self, mask: torch.Tensor) -> dict:
        idx = self.k.compact_index(mask)
        out = self.k.gather_rows([self.params[k] for k in GROUPS], idx)
        return dict(zip(GROUPS, out))

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        scaling = torch.exp(self.params["scaling"])
        mask = (grads >= grad_threshold) & (scaling.max(dim=1).values <= self.percent_dense * scene_extent)
        self._append(self._rows(mask))

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, samples=None):
        n_init = self.num_points
        padded = torch.zeros(n_init, dtype=torch.float32, device=self.device)
        padded[: grads.shape[0]] = grads
        scaling = torch.exp(self.params["scaling"])
        mask = (padded >= grad_threshold) & (scaling.max(dim=1).values > self.percent_dense * scene_extent)
        sel = self._rows(mask)
        stds = torch.exp(sel["scaling"]).repeat(N, 1)
        if samples is None:
            samples = torch.normal(torch.zeros_like(stds), stds, generator=self.gen)
        rots = build_rotation(sel["rotation"]).repeat(N, 1, 1)
        new = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + sel["xyz"].repeat(N, 1),
               "scaling": torch.log(torch.exp(sel["scaling"]).repeat(N, 1) / (0.8 * N)),
               "rotation": sel["rotation"].repeat(N, 1), "f_dc": sel["f_dc"].repeat(N, 1, 1),
               "f_rest": sel["f_rest"].repeat(N, 1, 1), "opacity": sel["opacity"].repeat(N, 1)}
        self._append(new)
        prune = torch.cat([mask, torch.zeros(N * int(sel["xyz"].shape[0]), dtype=torch.bool, device=self.device)])
        self.prune_points(prune)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, split_samples=None):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent, samples=split_samples)
        prune = (torch.sigmoid(self.params["opacity"]) < min_opacity).squeeze(1)
        if max_screen_size:
            big_vs = self.max_radii2D > max_screen_size
            big_ws = torch.exp(self.params["scaling"]).max(dim=1).values > 0.1 * extent
            prune = prune | big_vs | big_ws
        self.prune_points(prune)

    def reset_opacity(self):
        o = torch.sigmoid(self.params["opacity"])
        o = torch.minimum(o, torch.full_like(o, 0.01))
        self.params["opacity"] = torch.log(o / (1 - o)).contiguous()  # inverse_sigmoid
        self.exp_avg["opacity"].zero_()
        self.exp_avg_sq["opacity"].zero_()
