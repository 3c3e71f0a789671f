#!/usr/bin/env python3
"""Cost of the trained per-view exposure on one GPU: the two fused kernels, and the step with it.

    python scripts/exposure_cost.py [--config 1m_1080p] [--reps 200] [--steps 20] [--rounds 5] [--out FILE.json]

(a) gsr_exposure_forward (3 planes read, 3 written: 24 B per pixel) and gsr_exposure_backward (6
    read, 3 written, plus the 12 sums: 36 B per pixel) on a 3 x H x W image with the clamp flag,
    against the torch-eager composition of the same values (upstream's permute / matmul / permute /
    add / clamp, and the gradients in closed form -- no autograd graph, which favours eager).  Each
    variant: warm-up, then `reps` back-to-back calls between two device events; the variants are
    interleaved round by round.  The byte floor is those bytes at DESIGN's copy rate.
(b) GaussianTrainer.step at the config's size with opt.train_exposure on and off (densify=False),
    two trainers on the same scene, interleaved round by round, wall clock between two device
    synchronisations.  Every learning rate is 0, the exposure's too, so both trainers render the
    same, unchanging scene in every step and every Adam launch still runs at full cost.
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
COPY_TBS = 6.29  # the measured copy rate DESIGN.md section 9a quotes
E = [[0.90, 0.25, -0.30, 0.12], [-0.35, 1.10, 0.20, -0.15], [0.30, -0.25, 0.80, 0.20]]


def eager_forward(img, exposure, clamp):
    y = torch.matmul(img.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
    return y.clamp(0.0, 1.0) if clamp else y


def eager_backward(img, exposure, dout, clamp):
    """The gradients of eager_forward composed from torch ops (what autograd would launch, without its graph)."""
    g = dout
    if clamp:
        y = torch.matmul(img.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
        g = dout * ((y >= 0.0) & (y <= 1.0))
    gp = g.permute(1, 2, 0)
    dimg = torch.matmul(gp, exposure[:3, :3].t()).permute(2, 0, 1)
    dE = torch.empty_like(exposure)
    dE[:, :3] = torch.matmul(img.reshape(3, -1), g.reshape(3, -1).t())
    dE[:, 3] = g.sum(dim=(1, 2))
    return dimg, dE


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
    img = t(rng.uniform(-0.25, 1.25, (3, H, W)))
    dout = t(rng.standard_normal((3, H, W)))
    exposure = t(E)

    variants = {
        "kernel_forward": lambda: K.exposure_forward(img, exposure, clamp=True),
        "eager_forward": lambda: eager_forward(img, exposure, True),
        "kernel_backward": lambda: K.exposure_backward(img, exposure, dout, clamp=True),
        "eager_backward": lambda: eager_backward(img, exposure, dout, True),
    }
    # the two agree before anything is timed (a pixel whose y rounds to the other side of a clamp
    # bound differs by one gradient element: compare the reductions and the bulk)
    ok, oe = variants["kernel_forward"](), variants["eager_forward"]()
    assert float((ok - oe).abs().max()) <= 1e-5, float((ok - oe).abs().max())
    (dk, ek), (de, ee) = variants["kernel_backward"](), variants["eager_backward"]()
    assert float(((dk - de).abs() > 1e-5).float().mean()) <= 1e-5
    assert float((ek - ee).abs().max()) <= 1e-5 * n, (ek, ee)  # the sums' absolute terms add up to about 0.4 n
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
    bytes_px = {"forward": 24, "backward": 36}
    floor = {k: round(b * n / (COPY_TBS * 1e12) * 1e3, 5) for k, b in bytes_px.items()}
    out = dict(what="exposure_cost", config=args.config, H=H, W=W, reps=args.reps, rounds=args.rounds,
               exposure_ms=kern, bytes_per_pixel=bytes_px, byte_floor_ms=floor, copy_tb_s=COPY_TBS,
               note="kernel_forward is one gsr_exposure_forward call and one torch.empty; kernel_backward one "
                    "gsr_exposure_backward call (the pass and the one-block finalize) and three torch.empty",
               eager_over_kernel={m: round(kern["eager_" + m]["mean"] / kern["kernel_" + m]["mean"], 3) for m in bytes_px},
               kernel_over_floor={m: round(kern["kernel_" + m]["mean"] / floor[m], 3) for m in bytes_px},
               device=torch.cuda.get_device_name(0), label=args.label)

    if not args.skip_step:
        cam = graphics.synthetic_camera(W, H)
        s = scene_mod.make_scene(cam, c["P"], max_sh_degree=3, seed=0)
        gt = t(rng.random((3, H, W)))
        frozen = dict(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0,
                      rotation_lr=0.0, exposure_lr_init=0.0, exposure_lr_final=0.0)

        def make(**kw):
            tr = trainer.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                                         s.raw_rotations, max_sh_degree=3,
                                         opt=trainer.OptimizationParams(**frozen, **kw), device=dev)
            tr.active_sh_degree = c["D"]
            return tr

        plain, exposed = make(), make(train_exposure=True)
        exposed.setup_exposure(200)  # a Mip-NeRF360-sized set of views: the whole tensor takes the Adam step
        exposed.exposure[7] = exposure
        it = {"plain": 0, "exposed": 0}

        def step_plain():
            it["plain"] += 1
            plain.step(it["plain"], cam, gt, densify=False)

        def step_exposed():
            it["exposed"] += 1
            exposed.step(it["exposed"], cam, gt, densify=False, view_index=7)

        steps = {"plain": step_plain, "exposed": step_exposed}
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
        for tr in (plain, exposed):
            tr.binning.poll()
        out.update(P=c["P"], steps=args.steps, views=200, step_ms=summ,
                   exposed_over_plain=round(summ["exposed"]["mean"] / summ["plain"]["mean"], 4),
                   exposed_minus_plain_ms=round(summ["exposed"]["mean"] - summ["plain"]["mean"], 4),
                   binning=dict(overflows=[plain.binning.overflows, exposed.binning.overflows],
                                exact_reads=[plain.binning.exact_reads, exposed.binning.exact_reads]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
