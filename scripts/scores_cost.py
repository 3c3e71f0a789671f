#!/usr/bin/env python3
"""Cost of the importance scores on one GPU: the replay and its gather beside F6, B1 and B1's gather.

    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \\
        python scripts/scores_cost.py --trace-only
    python scripts/scores_cost.py --kernel-stats DIR/.../trace_kernel_stats.csv --out FILE.json

(a) One kernel trace holding all five: --trace-only renders the config's scene and runs `reps` rounds
    of forward, backward and scores under rocprofv3; --kernel-stats reads that run's kernel_stats.csv
    and records the average duration of blend_forward_kernel (F6), blend_backward_kernel (B1),
    gather_grad2d_kernel, score_replay_kernel and score_gather_kernel.
(b) Without a profiler, between device events: the whole gsr_forward_scores call (flag clear, replay,
    gather, the scratch allocation through the callback) beside gsr_forward and gsr_backward on the
    same scene, interleaved round by round.
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

import torch  # noqa: E402

PKG = "3d_gaussian_splatting_amd"
graphics = importlib.import_module(f"{PKG}.graphics")
scene_mod = importlib.import_module(f"{PKG}.scene")
rasterizer = importlib.import_module(f"{PKG}.rasterizer")

CONFIGS = {"1m_1080p": dict(P=1_000_000, W=1920, H=1080, D=3), "100k_800": dict(P=100_000, W=800, H=800, D=3)}
KERNELS = {"f6": "blend_forward_kernel", "b1": "blend_backward_kernel", "gather_grad2d": "gather_grad2d_kernel",
           "score_replay": "score_replay_kernel", "score_gather": "score_gather_kernel"}


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
    """{kernel: (calls, average microseconds)} from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for key, needle in KERNELS.items():
                if needle in name:
                    c0, t0 = out.get(key, (0, 0.0))
                    out[key] = (c0 + int(float(row["Calls"])), t0 + float(row["TotalDurationNs"]))
    return {k: dict(calls=c, avg_us=round(t / c / 1e3, 3)) for k, (c, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--trace-only", action="store_true", help="part (a)'s workload, for a run under rocprofv3")
    ap.add_argument("--kernel-stats", default=None, help="that run's kernel_stats.csv, recorded with (b)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="recorded as is (e.g. the commit and machine measured)")
    args = ap.parse_args()
    c = CONFIGS[args.config]
    dev = torch.device("cuda", 0)
    cam = graphics.synthetic_camera(c["W"], c["H"])
    s = scene_mod.make_scene(cam, c["P"], max_sh_degree=3, seed=0)
    rast = rasterizer.CAbiRasterizer(dev)
    dpix = torch.as_tensor(scene_mod.make_dL_dpix(cam), device=dev)
    inputs = [torch.as_tensor(a, device=dev) for a in (s.means3D, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest)]
    forward = lambda: rast.forward(cam, *inputs, sh_degree=c["D"])
    st = forward()
    sc = rast.scores(st)
    used = int((sc["hits"] > 0).sum())
    variants = {"forward": forward, "backward": lambda: rast.backward(st, dpix), "scores": lambda: rast.scores(st)}

    if args.trace_only:
        for _ in range(args.reps):
            for f in variants.values():
                f()
        torch.cuda.synchronize()
        print(json.dumps(dict(what="scores_trace", config=args.config, reps=args.reps, used=used)))
        return

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
    out = dict(what="scores_cost", config=args.config, P=c["P"], H=c["H"], W=c["W"], sh_degree=c["D"],
               num_rendered=st.num_rendered, visible=int((st.radii > 0).sum()), used=used,
               below_radsplat_threshold=int(((sc["max_w"] < 0.01) & (st.radii > 0)).sum()),
               reps=args.reps, rounds=args.rounds, call_ms={k: summarise(v) for k, v in ms.items()},
               note="call_ms are whole C-ABI calls between device events, their torch.empty outputs and scratch "
                    "included: forward = gsr_forward (exact sizing: one host read), backward = gsr_backward, "
                    "scores = gsr_forward_scores (flag clear, replay, gather)",
               device=torch.cuda.get_device_name(0), label=args.label)
    if args.kernel_stats:
        ks = read_kernel_stats(args.kernel_stats)
        out["kernel_trace"] = ks
        if set(KERNELS) <= set(ks):
            out["scores_kernels_us"] = round(ks["score_replay"]["avg_us"] + ks["score_gather"]["avg_us"], 3)
            out["b1_plus_gather_us"] = round(ks["b1"]["avg_us"] + ks["gather_grad2d"]["avg_us"], 3)
            out["replay_over_f6"] = round(ks["score_replay"]["avg_us"] / ks["f6"]["avg_us"], 4)
            out["replay_over_b1"] = round(ks["score_replay"]["avg_us"] / ks["b1"]["avg_us"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
