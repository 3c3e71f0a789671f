#!/usr/bin/env python3
"""Cost of anti-aliased rendering (GSR_FLAG_ANTIALIAS) on one GPU.

    python scripts/antialias_cost.py [--config 1m_1080p] [--steps 20] [--rounds 5] [--out FILE.json]

Two steps on bench.py's scene (same seed, same binning bound, every call through the C ABI):
  plain      forward + backward
  antialias  forward(antialiasing=True) + backward of its state
interleaved round by round (measuring guide: one process, alternating variants, so clock and thermal
drift hit both alike); each round times `steps` steps by wall clock between two device
synchronisations, and -- in a second, untimed-by-wall-clock set of rounds, interleaved the same way --
the library's stage events give every stage per step and round.

Only F1 (preprocess) and B2 (preprocess_bwd) are like for like: the flag changes those two kernels
alone, and K, the sorted list and the ranges are bit-identical.  The flagged scene blends lower
opacities, so F6, B1 and the gather visit fewer records: their times are reported, not a speed-up of
the feature.  Prints one JSON line; --out also writes it.
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

import torch  # noqa: E402

PKG = "3d_gaussian_splatting_amd"
native = importlib.import_module(f"{PKG}.native")
R = importlib.import_module(f"{PKG}.rasterizer")
graphics = importlib.import_module(f"{PKG}.graphics")
scene_mod = importlib.import_module(f"{PKG}.scene")
bands = importlib.import_module(f"{PKG}.bands")

CONFIGS = {"1m_1080p": dict(P=1_000_000, W=1920, H=1080, D=3), "100k_800": dict(P=100_000, W=800, H=800, D=3)}
LIKE_FOR_LIKE = ("preprocess", "preprocess_bwd")


def _summary(v):
    return dict(mean=round(statistics.mean(v), 5), min=round(min(v), 5), max=round(max(v), 5),
                rounds=[round(x, 5) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="recorded as is (e.g. the commit and machine measured)")
    args = ap.parse_args()
    c = CONFIGS[args.config]
    dev = torch.device("cuda", 0)
    cam = graphics.synthetic_camera(c["W"], c["H"])
    s = scene_mod.make_scene(cam, c["P"], max_sh_degree=3, seed=0)
    t = lambda a: torch.tensor(a, device=dev)
    inputs = dict(means3D=t(s.means3D), opacities=t(s.opacities), scales=t(s.scales), rotations=t(s.rotations),
                  sh_dc=t(s.sh_dc), sh_rest=t(s.sh_rest))
    dC = t(scene_mod.make_dL_dpix(cam, seed=1))
    rast = R.CAbiRasterizer(dev)
    st0 = rast.forward(cam, **inputs, sh_degree=c["D"])
    K = st0.num_rendered
    cap = bands.round_up(int(K * 1.1) + 1)
    st1 = rast.forward(cam, **inputs, sh_degree=c["D"], antialiasing=True)
    assert st1.num_rendered == K and torch.equal(st0.radii, st1.radii)  # the flag moves no discrete output
    # how far the flag moves the opacities of this scene (the blend stages' work follows them)
    P = c["P"]
    o0 = st0.view(native.VIEW_RECORDS, torch.float32, 12 * P).view(P, 3, 4)[:, 1, 1]
    o1 = st1.view(native.VIEW_RECORDS, torch.float32, 12 * P).view(P, 3, 4)[:, 1, 1]
    vis = st0.radii > 0
    coef = (o1[vis] / o0[vis]).double()
    coef_stats = dict(mean=round(float(coef.mean()), 4), min=round(float(coef.min()), 5),
                      below_half=round(float((coef < 0.5).double().mean()), 4))
    del st0, st1

    def step(aa):
        st = rast.forward(cam, **inputs, sh_degree=c["D"], max_rendered=cap, antialiasing=aa)
        return rast.backward(st, dC)

    variants = dict(plain=lambda: step(False), antialias=lambda: step(True))
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
    stage_rounds = {k: {s_: [] for s_ in native.STAGES} for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            native.profile_enable()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            got = native.profile_read()
            native.profile_enable(0)
            for s_ in native.STAGES:
                stage_rounds[name][s_].append(got[s_][0] / args.steps)
    stages = {k: {s_: _summary(v) for s_, v in d.items() if max(v) > 0} for k, d in stage_rounds.items()}
    summ = {k: _summary(v) for k, v in ms.items()}
    like = {s_: dict(plain=stages["plain"][s_]["mean"], antialias=stages["antialias"][s_]["mean"],
                     ratio=round(stages["antialias"][s_]["mean"] / stages["plain"][s_]["mean"], 4),
                     plain_spread=round(stages["plain"][s_]["max"] - stages["plain"][s_]["min"], 5))
            for s_ in LIKE_FOR_LIKE}
    out = dict(what="antialias_cost", config=args.config, P=c["P"], W=c["W"], H=c["H"], sh_degree=c["D"],
               num_rendered=K, capacity=cap, steps=args.steps, rounds=args.rounds, coef_of_visible=coef_stats,
               ms_per_step=summ, stage_ms_per_step=stages, like_for_like=like,
               antialias_over_plain=round(summ["antialias"]["mean"] / summ["plain"]["mean"], 4),
               device=torch.cuda.get_device_name(0), label=args.label)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
