#!/usr/bin/env python3
"""Cost of the depth / alpha outputs (gsr_forward_aux / gsr_backward_aux) on one GPU.

    python scripts/aux_cost.py [--config 1m_1080p] [--steps 20] [--rounds 5] [--out FILE.json]

Three steps on bench.py's scene (same seed, same binning bound, every call through the C ABI):
  plain     forward + backward                                  (colour only)
  aux       forward_aux + backward_aux                          (colour, depth, alpha: one pass)
  two_pass  plain, then a second forward + backward with colors_precomp = (z, 1, 0) and
            dL/dcolor = (dL/ddepth, dL/dalpha, 0) -- the workaround without the aux calls (its
            colours are prepared once, outside the timed steps, and the dL/dz -> dL/dmeans3D term
            the caller would still have to apply is left out: both favour the workaround)
The variants are interleaved round by round (measuring guide: one process, alternating builds /
variants, so clock and thermal drift hit all alike); each round times `steps` steps by wall clock
between two device synchronisations.  Then one untimed pass per variant with the library's stage
events gives F6 / B1 / gather / B2 per step.  Prints one JSON line; --out also writes it.
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
native = importlib.import_module(f"{PKG}.native")
R = importlib.import_module(f"{PKG}.rasterizer")
graphics = importlib.import_module(f"{PKG}.graphics")
scene_mod = importlib.import_module(f"{PKG}.scene")
bands = importlib.import_module(f"{PKG}.bands")

CONFIGS = {"1m_1080p": dict(P=1_000_000, W=1920, H=1080, D=3), "100k_800": dict(P=100_000, W=800, H=800, D=3)}
STAGES = ("blend_fwd", "blend_bwd", "gather_grad2d", "preprocess_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=3.0)
    ap.add_argument("--inverse-depth", action="store_true")
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
    rng = np.random.default_rng(2)
    dD = t(rng.uniform(-1, 1, (c["H"], c["W"])).astype(np.float32))
    dA = t(rng.uniform(-1, 1, (c["H"], c["W"])).astype(np.float32))
    rast = R.CAbiRasterizer(dev)
    st0 = rast.forward(cam, **inputs, sh_degree=c["D"])
    K = st0.num_rendered
    cap = bands.round_up(int(K * 1.1) + 1)
    # the workaround's second pass: colours (v, 1, 0) from F1's own depth, 0 where culled
    z = st0.view(native.VIEW_DEPTH_KEY, torch.int32, c["P"]).view(torch.float32)
    vis = st0.radii > 0
    v = torch.where(vis, (1.0 / z) if args.inverse_depth else z, torch.zeros_like(z))
    aux_cols = torch.stack([v, vis.float(), torch.zeros_like(v)], 1).contiguous()
    geom = {k: inputs[k] for k in ("means3D", "opacities", "scales", "rotations")}
    dpix2 = torch.stack([dD, dA, torch.zeros_like(dD)]).contiguous()
    del st0

    def plain():
        st = rast.forward(cam, **inputs, sh_degree=c["D"], max_rendered=cap)
        return rast.backward(st, dC)

    def aux():
        st = rast.forward_aux(cam, **inputs, sh_degree=c["D"], max_rendered=cap, inverse_depth=args.inverse_depth)
        return rast.backward_aux(st, dC, dD, dA)

    def two_pass():
        plain()
        st = rast.forward(cam, **geom, colors_precomp=aux_cols, sh_degree=0, max_rendered=cap)
        return rast.backward(st, dpix2)

    variants = dict(plain=plain, aux=aux, two_pass=two_pass)
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
    stages = {}
    for name in ("plain", "aux"):
        native.profile_enable()
        for _ in range(args.steps):
            variants[name]()
        torch.cuda.synchronize()
        got = native.profile_read()
        native.profile_enable(0)
        stages[name] = {k: round(got[k][0] / args.steps, 5) for k in STAGES}
    summ = {k: dict(mean=round(statistics.mean(v), 4), min=round(min(v), 4), max=round(max(v), 4),
                    rounds=[round(x, 4) for x in v]) for k, v in ms.items()}
    out = dict(what="aux_cost", config=args.config, P=c["P"], W=c["W"], H=c["H"], sh_degree=c["D"],
               inverse_depth=args.inverse_depth, num_rendered=K, capacity=cap, steps=args.steps, rounds=args.rounds,
               ms_per_step=summ, stage_ms_per_step=stages,
               aux_over_plain=round(summ["aux"]["mean"] / summ["plain"]["mean"], 4),
               two_pass_over_aux=round(summ["two_pass"]["mean"] / summ["aux"]["mean"], 4),
               device=torch.cuda.get_device_name(0), label=args.label)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
