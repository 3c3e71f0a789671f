#!/usr/bin/env python3
"""Cost of the visibility-masked Adam step (gsr_adam_step_sparse) against the dense one on one GPU.

    python scripts/sparse_adam_cost.py [--P 1000000] [--steps 20] [--rounds 5] [--out FILE.json]

Six groups of P Gaussians with the SH3 row widths (3, 3, 45, 1, 3, 4 floats) and the trainer's
activations.  The dense step and the sparse step under each mask run on the same arrays, interleaved
round by round in one process (measuring guide: alternating variants, so clock and thermal drift hit
all alike); each round times `steps` steps by wall clock between two device synchronisations.

Masks (share of Gaussians with radii > 0):
  all            every Gaussian visible: the sparse step does the dense step's work plus the radii reads
  random50/10    independent per Gaussian
  runs50/10      runs of 4096 consecutive Gaussians, each run visible as a whole or not at all
  camera         the radii of one forward of bench.py's scene (same seed, P Gaussians, 1080p) from a
                 camera moved 3 units into the cloud, which then sees part of it; the scene's indices
                 carry no spatial order, so this mask is spatially random in memory

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
R = importlib.import_module(f"{PKG}.rasterizer")
graphics = importlib.import_module(f"{PKG}.graphics")
scene_mod = importlib.import_module(f"{PKG}.scene")

WIDTHS = {"xyz": 3, "f_dc": 3, "f_rest": 45, "opacity": 1, "scaling": 3, "rotation": 4}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
RUN = 4096


def _summary(v):
    return dict(mean=round(statistics.mean(v), 5), min=round(min(v), 5), max=round(max(v), 5),
                rounds=[round(x, 5) for x in v])


def camera_radii(P, dev):
    """radii of bench.py's scene seen from (0, 0, 3), looking down +z like the scene's own camera."""
    cam0 = graphics.synthetic_camera(1920, 1080)
    s = scene_mod.make_scene(cam0, P, max_sh_degree=3, seed=0)
    fovx = 2.0 * np.arctan(cam0.tanfovx)
    fovy = 2.0 * np.arctan(cam0.tanfovy)
    cam = graphics.make_camera(np.eye(3), np.array([0.0, 0.0, -3.0]), fovx, fovy, 1920, 1080)
    t = lambda a: torch.tensor(a, device=dev)
    st = R.CAbiRasterizer(dev).forward(cam, t(s.means3D), t(s.opacities), scales=t(s.scales), rotations=t(s.rotations),
                                       sh_dc=t(s.sh_dc), sh_rest=t(s.sh_rest), sh_degree=3)
    return st.radii.clone().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="recorded as is (e.g. the commit and machine measured)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    P = args.P
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    r = lambda w, scale: torch.randn((P, w), generator=gen, device=dev) * scale
    groups = [dict(param=r(w, 1.0), grad=r(w, 1e-3), exp_avg=r(w, 1e-3), exp_avg_sq=r(w, 1e-3) ** 2,
                   act=trainer.ACTS[k], step=100, lr=LRS[k]) for k, w in WIDTHS.items()]
    floats = sum(WIDTHS.values())

    def to_radii(rows):
        return rows.to(torch.int32).contiguous()

    n_runs = (P + RUN - 1) // RUN
    run_rows = lambda share: (torch.rand(n_runs, generator=gen, device=dev) < share).repeat_interleave(RUN)[:P]
    masks = {"all": torch.ones(P, dtype=torch.int32, device=dev),
             "random50": to_radii(torch.rand(P, generator=gen, device=dev) < 0.5),
             "random10": to_radii(torch.rand(P, generator=gen, device=dev) < 0.1),
             "runs50": to_radii(run_rows(0.5)), "runs10": to_radii(run_rows(0.1)),
             "camera": camera_radii(P, dev)}
    share = {k: round(float((m > 0).double().mean()), 4) for k, m in masks.items()}
    K = trainer.TrainKernels(dev)
    variants = {"dense": lambda: K.adam_step(groups)}
    for name, m in masks.items():
        variants["sparse_" + name] = (lambda m=m: K.adam_step(groups, visibility=m))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup_s:
        for f in variants.values():
            f()
        torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            torch.cuda.synchronize()
            a = time.perf_counter()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - a) / args.steps)
    summ = {k: _summary(v) for k, v in ms.items()}
    dense = summ["dense"]
    # the one derived expectation: all visible <= dense x 1.015 (6 x 4 B of radii on 1652 B per
    # Gaussian) plus the dense step's own min-max spread of this run
    bound = round(dense["mean"] * 1.015 + (dense["max"] - dense["min"]), 5)
    out = dict(what="sparse_adam_cost", P=P, floats_per_gaussian=floats, bytes_per_gaussian_dense=28 * floats,
               steps=args.steps, rounds=args.rounds, run_length=RUN, visible_share=share, ms_per_step=summ,
               over_dense={k: round(v["mean"] / dense["mean"], 4) for k, v in summ.items()},
               all_visible_bound_ms=bound, all_visible_within_bound=bool(summ["sparse_all"]["mean"] <= bound),
               device=torch.cuda.get_device_name(0), label=args.label)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
