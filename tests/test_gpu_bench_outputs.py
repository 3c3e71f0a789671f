"""GPU: what a bench.py run does and writes.

A plain run times its steps and prints the headline line only; --dump-outputs DIR writes the last
timed step's outputs, which must be exactly what a caller of the same path (CAbiRasterizer forward
+ backward on the same seeded scene) receives; --full adds the stage pass, the roofline figures and
the CPU oracle's baseline / parity leg.  The plain run uses the smallest config (1k Gaussians,
256x256), the --full run the smallest with SH degree 3 (100k Gaussians, 800x800), which its parity
leg's gradient list is written for.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("stage_ms", "stage_hbm_frac", "roofline", "pipeline_roofline", "cpu_baseline", "parity")


def _bench(args, config="1k_256"):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", config] + args, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_what_the_step_returns(tmp_path):
    import bench
    out = tmp_path / "out"
    j = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    for k in HEADLINE:
        assert k in j, k
    assert j["steps"] == 3 and j["n_gpus"] == 1 and j["unit"] == "iters/s" and j["higher_is_better"] is True
    assert j["metric"] == bench.config_metric("1k_256")
    assert j["ms_per_step"] > 0 and abs(j["value"] - 1e3 / j["ms_per_step"]) <= 1e-2 * j["value"]
    for k in FULL_ONLY:
        assert k not in j, k

    cfg = bench.CONFIGS["1k_256"]
    gr, sc, R = pkg("graphics"), pkg("scene"), pkg("rasterizer")
    cam = gr.synthetic_camera(cfg["W"], cfg["H"])
    s = sc.make_scene(cam, cfg["P"], max_sh_degree=cfg["D"], seed=0)
    rast = R.CAbiRasterizer("cuda:0")
    st = rast.forward(cam, s.means3D, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest, sh_degree=cfg["D"])
    g = rast.backward(st, sc.make_dL_dpix(cam, seed=1))
    torch.cuda.synchronize()
    want = {"color": st.color, "radii": st.radii, **g}
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == sorted(want)  # all of it fits: no sample
    assert int((st.radii > 0).sum()) > 0
    for k, t in want.items():
        assert got[k].dtype == np.float32, k
        np.testing.assert_array_equal(got[k], t.cpu().numpy().astype(np.float32), err_msg=k)


def test_full_run_adds_the_other_measurements():
    j = _bench(["--steps", "3", "--warmup", "1", "--full"], config="100k_800")
    for k in HEADLINE + FULL_ONLY:
        assert k in j, k
    assert j["steps"] == 3 and j["parity"]["num_rendered_equal"] is True
    assert j["parity"]["psnr_db_vs_cpu"] >= 50.0 and j["parity"]["grad_rel_l2_max"] <= 1e-4
