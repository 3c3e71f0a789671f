"""Depth supervision without a GPU: the gsr_depth_loss ABI (declared, listed, exported, scratch
sizing, argument validation -- every check returns before a device call), upstream's
depth_params.json inputs (scene_io) and the trainer's depth options and weight schedule."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, pkg

TRAIN_HEADER = os.path.join(ROOT, "include", "gsr", "gsr_train.h")
NEW = ["gsr_depth_loss_scratch_bytes", "gsr_depth_loss"]


def test_symbols_declared_listed_and_exported():
    native = pkg("native")
    text = open(TRAIN_HEADER).read()
    for f in NEW:
        assert re.search(rf"^\s*(?:size_t|int)\s+{f}\s*\(", text, re.M), f
        assert f in native.TRAIN_EXPORTS
    val = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert val("GSR_DEPTH_RAW") == native.DEPTH_RAW == 0
    assert val("GSR_DEPTH_NORMALIZED") == native.DEPTH_NORMALIZED == 1
    out = subprocess.run(["nm", "-D", "--defined-only", native.hip_library_path()], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW if f not in syms]
    assert native.load_hip().gsr_abi_version() == native.ABI_VERSION == 4  # new symbols only


def test_scratch_bytes_positive_and_monotone():
    L = pkg("native").load_hip()
    shapes = [(1, 1), (1, 3), (16, 16), (70, 101), (33, 200), (480, 640), (1080, 1920), (1024, 2049), (2160, 3840),
              (8192, 8192)]
    shapes.sort(key=lambda s: s[0] * s[1])
    sizes = [int(L.gsr_depth_loss_scratch_bytes(h, w)) for h, w in shapes]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] < sizes[-1]
    # one 8-byte (sum, count) partial per block; the grid is capped, so the scratch is too
    assert sizes[-1] <= 64 * 1024


def test_validation_without_gpu():
    native = pkg("native")
    L = native.load_hip()
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first
    RAW, NORM = native.DEPTH_RAW, native.DEPTH_NORMALIZED

    def call(depth=fake, alpha=fake, target=fake, mask=None, H=8, W=8, weight=1.0, mode=RAW, alpha_min=0.5,
             scratch=fake, stats=fake, dd=fake, da=fake):
        return L.gsr_depth_loss(depth, alpha, target, mask, H, W, weight, mode, alpha_min, scratch, stats, dd, da, None)

    bad = [dict(H=0), dict(W=0), dict(H=-3), dict(W=-1),
           dict(depth=None), dict(target=None), dict(scratch=None), dict(stats=None), dict(dd=None),
           dict(mode=2), dict(mode=-1),
           dict(mode=NORM, alpha=None), dict(mode=NORM, da=None),
           dict(mode=NORM, alpha_min=0.0), dict(mode=NORM, alpha_min=-0.5),
           dict(weight=-1.0), dict(weight=float("inf")), dict(weight=float("nan"))]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert "depth loss" in native.last_error(), (kw, native.last_error())


def test_depth_params_and_target(tmp_path):
    sio = pkg("scene_io")
    path = tmp_path / "depth_params.json"
    raw = {"a.jpg": {"scale": 2.0, "offset": 0.25}, "b.jpg": {"scale": 1.0, "offset": -0.5},
           "c.jpg": {"scale": 3.0, "offset": 0.0}, "far.jpg": {"scale": 40.0, "offset": 0.1},
           "neg.jpg": {"scale": -1.0, "offset": 0.0}}
    path.write_text(json.dumps(raw))
    dp = sio.load_depth_params(str(path))
    assert set(dp) == set(raw)
    med = float(np.median([2.0, 1.0, 3.0, 40.0]))  # upstream: the median of the positive scales
    for k, v in raw.items():
        assert dp[k]["scale"] == v["scale"] and dp[k]["offset"] == v["offset"] and dp[k]["med_scale"] == med
    img = np.arange(12, dtype=np.float32).reshape(3, 4) / 7
    t, ok = sio.depth_target(img, **dp["a.jpg"])
    assert ok and t.dtype == np.float32 and t.shape == (3, 4)
    np.testing.assert_array_equal(t, img * np.float32(2.0) + np.float32(0.25))
    assert sio.depth_target(img, **dp["far.jpg"])[1] is False      # 40 > 5 * 2.5
    assert sio.depth_target(img, **dp["neg.jpg"])[1] is False      # below 0.2 * med
    assert sio.depth_target(img, 0.5, 0.0, 2.5)[1] is True         # the lower edge, 0.2 * 2.5, is reliable
    assert sio.depth_target(img, 12.5, 0.0, 2.5)[1] is True        # the upper edge, 5 * 2.5, too
    assert sio.depth_target(img, 0.49, 0.0, 2.5)[1] is False


def test_optimization_params_and_schedule():
    T, general = pkg("trainer"), pkg("general")
    o = T.OptimizationParams()
    assert (o.depth_l1_weight_init, o.depth_l1_weight_final) == (1.0, 0.01)
    assert o.depth_inverse is True and o.depth_normalized is False and o.depth_alpha_min == 0.5
    f = general.get_expon_lr_func(o.depth_l1_weight_init, o.depth_l1_weight_final, max_steps=o.iterations)
    assert f(0) == o.depth_l1_weight_init
    assert math.isclose(f(o.iterations), o.depth_l1_weight_final, rel_tol=1e-12)
    assert math.isclose(f(o.iterations // 2), 0.1, rel_tol=1e-12)  # log-linear: the geometric mean half way
    assert general.get_expon_lr_func(0.0, 0.0, max_steps=o.iterations)(5) == 0.0  # both 0: no depth term
