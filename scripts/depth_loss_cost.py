#!/usr/bin/env python3
"""Cost of depth supervision on one GPU: the fused depth-loss kernel, and the supervised step.

    python scripts/depth_loss_cost.py [--config 1m_1080p] [--reps 200] [--steps 20] [--rounds 5] [--out FILE.json]

(a) gsr_depth_loss on an H x W plane, both modes (RAW: 3 planes read with a mask, 1 written;
    NORMALIZED: 4 read, 2 written), against the torch-eager composition of the same loss and
    gradients (abs / mul / mean / sign ... on the same device, gradients in closed form -- no
    autograd graph, which favours eager).  Each variant: warm-up, then `reps` back-to-back calls
    between two device events; the variants are interleaved round by round.  The byte floor is
    planes x 4 B x n at DESIGN's 8 TB/s HBM figure.
(b) GaussianTrainer.step at the config's size with and without a depth target (densify=False),
    two trainers on the same scene, interleaved round by round, wall clock between two device
    synchronisations.  Every learning rate is 0, so the fused Adam step runs at full cost but both
    trainers render the same, unchanging scene in every step (with the default rates the two
    scenes drift apart during the warm-up and the comparison measures the drift).
Prints one JSON line; --out also writes it.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PKG = "3d_gaussian_splatting_amd"
trainer = importlib.import_module(f"{PKG}.trainer")
graphics = importlib.import_module(f"{PKG}.graphics")
scene_mod = importlib.import_module(f"{PKG}.scene")

CONFIGS = {"1m_1080p": dict(P=1_000_000, W=1920, H=1080, D=3), "100k_800": dict(P=100_000, W=800, H=800, D=3)}
HBM_TBS = 8.0  # the rate DESIGN.md's byte floors use


def eager_depth_loss(depth, alpha, target, mask, weight, normalized, alpha_min):
    """The same loss and gradients composed from torch ops (what a caller writes without the kernel)."""
    n = depth.numel()
    if normalized:
        ok = alpha >= alpha_min
        a = torch.where(ok, alpha, torch.ones_like(alpha))
        m = mask * ok
        pred = depth / a
    else:
        m, pred = mask, depth
    e = (pred - target) * m
    l1 = e.abs().mean()
    gp = (weight / n) * m * torch.sign(e)
    if normalized:
        return weight * l1, gp / a, -gp * depth / (a * a)
    return weight * l1, gp, None


def time_calls(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summarise(v):
    return dict(mean=round(statistics.mean(v), 5), min=round(min(v), 5), max=round(max(v), 5),
                rounds=[round(x, 5) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--skip-step", action="store_true", help="part (a) only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="recorded as is (e.g. the commit and machine measured)")
    args = ap.parse_args()
    c = CONFIGS[args.config]
    H, W = c["H"], c["W"]
    n = H * W
    dev = torch.device("cuda", 0)
    K = trainer.TrainKernels(dev)
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    alpha = t(rng.uniform(0.0, 1.0, (H, W)))
    z = t(rng.uniform(0.1, 3.0, (H, W)))
    depth = z * alpha
    # targets at least 0.01 from the prediction of their mode, so the kernel and the eager
    # composition (which round the prediction differently) agree on every sign
    delta = t(rng.uniform(0.01, 0.5, (H, W)) * rng.choice([-1.0, 1.0], (H, W)))
    target = {"raw": depth + delta, "normalized": z + delta}
    mask = t((rng.random((H, W)) > 0.2).astype(np.float32))

    variants = {
        "kernel_raw": lambda: K.depth_loss(depth, target["raw"], mask=mask, weight=0.5),
        "eager_raw": lambda: eager_depth_loss(depth, None, target["raw"], mask, 0.5, False, 0.5),
        "kernel_normalized": lambda: K.depth_loss(depth, target["normalized"], mask=mask, alpha=alpha, weight=0.5,
                                                  normalized=True),
        "eager_normalized": lambda: eager_depth_loss(depth, alpha, target["normalized"], mask, 0.5, True, 0.5),
    }
    # the two agree before anything is timed
    for mode, norm in (("raw", False), ("normalized", True)):
        st, dd, da = variants["kernel_" + mode]()
        l, gd, ga = variants["eager_" + mode]()
        assert abs(float(st[0]) - float(l)) <= 1e-4 * abs(float(l)), (mode, float(st[0]), float(l))
        assert float((dd - gd).abs().max()) <= 1e-5 * float(gd.abs().max()), mode
        assert (not norm) or float((da - ga).abs().max()) <= 1e-5 * float(ga.abs().max()), mode
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup_s:
        for f in variants.values():
            f()
        torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            torch.cuda.synchronize()
            ms[name].append(time_calls(f, args.reps))
    kern = {k: summarise(v) for k, v in ms.items()}
    planes = {"raw": 3 + 1, "normalized": 4 + 2}  # read (depth, target, mask[, alpha]) + written
    floor = {k: round(p * 4 * n / (HBM_TBS * 1e12) * 1e3, 5) for k, p in planes.items()}
    out = dict(what="depth_loss_cost", config=args.config, H=H, W=W, reps=args.reps, rounds=args.rounds,
               depth_loss_ms=kern, byte_floor_ms=floor, hbm_tb_s=HBM_TBS,
               note="kernel_* is one gsr_depth_loss call: the pass, the one-block finalize and three torch.empty",
               eager_over_kernel={m: round(kern["eager_" + m]["mean"] / kern["kernel_" + m]["mean"], 3) for m in planes},
               kernel_over_floor={m: round(kern["kernel_" + m]["mean"] / floor[m], 3) for m in planes},
               device=torch.cuda.get_device_name(0), label=args.label)

    if not args.skip_step:
        cam = graphics.synthetic_camera(W, H)
        s = scene_mod.make_scene(cam, c["P"], max_sh_degree=3, seed=0)
        gt = t(rng.random((3, H, W)))

        frozen = trainer.OptimizationParams(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0,
                                            scaling_lr=0.0, rotation_lr=0.0)

        def make():
            tr = trainer.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                                         s.raw_rotations, max_sh_degree=3, opt=frozen, device=dev)
            tr.active_sh_degree = c["D"]
            return tr

        colour, sup = make(), make()
        probe = sup.rast.forward_aux(cam, t(s.means3D), t(s.opacities).reshape(-1), scales=t(s.scales),
                                     rotations=t(s.rotations), sh_dc=t(s.sh_dc), sh_rest=t(s.sh_rest),
                                     sh_degree=c["D"], inverse_depth=True)
        gt_depth = (probe.depth * t(rng.uniform(0.8, 1.2, (H, W)))).contiguous()
        del probe
        it = {"colour": 0, "supervised": 0}

        def step_colour():
            it["colour"] += 1
            colour.step(it["colour"], cam, gt, densify=False)

        def step_sup():
            it["supervised"] += 1
            sup.step(it["supervised"], cam, gt, densify=False, gt_depth=gt_depth, depth_mask=mask)

        steps = {"colour": step_colour, "supervised": step_sup}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warmup_s:
            for f in steps.values():
                f()
            torch.cuda.synchronize()
        sms = {k: [] for k in steps}
        for _ in range(args.rounds):
            for name, f in steps.items():
                torch.cuda.synchronize()
                a = time.perf_counter()
                for _ in range(args.steps):
                    f()
                torch.cuda.synchronize()
                sms[name].append(1e3 * (time.perf_counter() - a) / args.steps)
        summ = {k: summarise(v) for k, v in sms.items()}
        for tr in (colour, sup):
            tr.binning.poll()
        out.update(P=c["P"], steps=args.steps, step_ms=summ,
                   supervised_over_colour=round(summ["supervised"]["mean"] / summ["colour"]["mean"], 4),
                   supervised_minus_colour_ms=round(summ["supervised"]["mean"] - summ["colour"]["mean"], 4),
                   binning=dict(overflows=[colour.binning.overflows, sup.binning.overflows],
                                exact_reads=[colour.binning.exact_reads, sup.binning.exact_reads]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
