#!/usr/bin/env python3
"""Cost of the camera gradients on one GPU: the camera pass against B2, and the step with it.

    python scripts/camera_grad_cost.py [--config 1m_1080p] [--reps 20] [--steps 20] [--rounds 5] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \\
        python scripts/camera_grad_cost.py --trace-only
    python scripts/camera_grad_cost.py --kernel-stats DIR/.../trace_kernel_stats.csv --out FILE.json

(a) One kernel trace holding both: --trace-only renders the config's scene once and runs `reps`
    posed backwards (gsr_backward_posed: B1, the gather, B2, then camera_backward_kernel and
    camera_finalize_kernel on the same grad2d) under rocprofv3; --kernel-stats reads that run's
    kernel_stats.csv and records the average duration of preprocess_backward_kernel (B2) and of the two
    camera kernels.  The camera pass reads no more than B2 reads and writes nothing per Gaussian, so it
    must take no longer than B2.
(b) Without a profiler, between device events: backward() with and without camera_grad on the same
    forward state, and backward_camera() alone against backward_preprocess() alone on the same grad2d,
    interleaved round by round.
(c) GaussianTrainer.step with opt.train_poses on and off (densify=False, every learning rate 0, so both
    trainers render the same unchanging scene and every launch runs at full cost), wall clock between
    two device synchronisations, interleaved round by round.
Prints one JSON line; --out also writes it.
"""
from __future__ import annotations

import argparse
import csv
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
rasterizer = importlib.import_module(f"{PKG}.rasterizer")

CONFIGS = {"1m_1080p": dict(P=1_000_000, W=1920, H=1080, D=3), "100k_800": dict(P=100_000, W=800, H=800, D=3)}
KERNELS = {"b2": "preprocess_backward_kernel", "camera": "camera_backward_kernel", "finalize": "camera_finalize_kernel"}


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


def read_kernel_stats(path):
    """{b2 / camera / finalize: (calls, average microseconds)} from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for key, needle in KERNELS.items():
                if needle in name:
                    calls = int(float(row["Calls"]))
                    total = float(row["TotalDurationNs"])
                    c0, t0 = out.get(key, (0, 0.0))
                    out[key] = (c0 + calls, t0 + total)
    return {k: dict(calls=c, avg_us=round(t / c / 1e3, 3)) for k, (c, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--trace-only", action="store_true", help="part (a)'s workload, for a run under rocprofv3")
    ap.add_argument("--kernel-stats", default=None, help="that run's kernel_stats.csv, recorded with (b) and (c)")
    ap.add_argument("--skip-step", action="store_true", help="no part (c)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="recorded as is (e.g. the commit and machine measured)")
    args = ap.parse_args()
    c = CONFIGS[args.config]
    H, W = c["H"], c["W"]
    dev = torch.device("cuda", 0)
    cam = graphics.synthetic_camera(W, H)
    s = scene_mod.make_scene(cam, c["P"], max_sh_degree=3, seed=0)
    rast = rasterizer.CAbiRasterizer(dev)
    dpix = torch.as_tensor(scene_mod.make_dL_dpix(cam), device=dev)
    st = rast.forward(cam, s.means3D, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest, sh_degree=c["D"])
    visible = int((st.radii > 0).sum())

    if args.trace_only:
        for _ in range(args.reps):
            rast.backward(st, dpix, camera_grad=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(what="camera_grad_trace", config=args.config, reps=args.reps, visible=visible)))
        return

    g2 = rast.backward_blend(st, dpix)
    variants = {
        "backward": lambda: rast.backward(st, dpix),
        "backward_posed": lambda: rast.backward(st, dpix, camera_grad=True),
        "b2_alone": lambda: rast.backward_preprocess(st, g2),
        "camera_alone": lambda: rast.backward_camera(st, g2),
    }
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
    calls = {k: summarise(v) for k, v in ms.items()}
    out = dict(what="camera_grad_cost", config=args.config, P=c["P"], H=H, W=W, sh_degree=c["D"], visible=visible,
               reps=args.reps, rounds=args.rounds, call_ms=calls,
               posed_minus_plain_ms=round(calls["backward_posed"]["mean"] - calls["backward"]["mean"], 5),
               camera_over_b2_calls=round(calls["camera_alone"]["mean"] / calls["b2_alone"]["mean"], 4),
               note="call_ms are whole C-ABI calls between device events (their torch.empty outputs included): "
                    "b2_alone is gsr_backward_preprocess, camera_alone gsr_backward_camera (the pass and its "
                    "finalize)",
               device=torch.cuda.get_device_name(0), label=args.label)
    if args.kernel_stats:
        ks = read_kernel_stats(args.kernel_stats)
        out["kernel_trace"] = ks
        if {"b2", "camera", "finalize"} <= set(ks):
            cam_us = ks["camera"]["avg_us"] + ks["finalize"]["avg_us"]
            out["camera_plus_finalize_us"] = round(cam_us, 3)
            out["camera_over_b2_trace"] = round(cam_us / ks["b2"]["avg_us"], 4)

    if not args.skip_step:
        gt = torch.as_tensor(np.random.default_rng(0).random((3, H, W), np.float32), device=dev)
        frozen = dict(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0,
                      rotation_lr=0.0, pose_lr_init=0.0, pose_lr_final=0.0)

        def make(**kw):
            tr = trainer.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                                         s.raw_rotations, max_sh_degree=3,
                                         opt=trainer.OptimizationParams(**frozen, **kw), device=dev)
            tr.active_sh_degree = c["D"]
            return tr

        plain, posed = make(), make(train_poses=True)
        posed.setup_poses(200)  # a Mip-NeRF360-sized set of views
        it = {"plain": 0, "posed": 0}

        def step_plain():
            it["plain"] += 1
            plain.step(it["plain"], cam, gt, densify=False)

        def step_posed():  # the views in turn: a view's update is applied when it comes round again
            it["posed"] += 1
            posed.step(it["posed"], cam, gt, densify=False, view_index=it["posed"] % 200)

        steps = {"plain": step_plain, "posed": step_posed}
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
        for tr in (plain, posed):
            tr.binning.poll()
        out.update(steps=args.steps, views=200, step_ms=summ,
                   posed_over_plain=round(summ["posed"]["mean"] / summ["plain"]["mean"], 4),
                   posed_minus_plain_step_ms=round(summ["posed"]["mean"] - summ["plain"]["mean"], 4),
                   step_note="the posed steps take the 200 views in turn: a view's pending update (one float64 chain "
                             "and Adam row on the host) is applied when the view comes round again, its copy long landed",
                   binning=dict(overflows=[plain.binning.overflows, posed.binning.overflows],
                                exact_reads=[plain.binning.exact_reads, posed.binning.exact_reads]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
