"""Trained per-view exposure without a GPU: the gsr_exposure_* ABI (declared, listed, exported,
scratch sizing, argument validation -- every check returns before a device call), upstream's
exposure.json (scene_io) and the trainer's exposure options and learning-rate schedule."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

TRAIN_HEADER = os.path.join(ROOT, "include", "gsr", "gsr_train.h")
NEW = ["gsr_exposure_scratch_bytes", "gsr_exposure_forward", "gsr_exposure_backward"]


def test_symbols_declared_listed_and_exported():
    native = pkg("native")
    text = open(TRAIN_HEADER).read()
    for f in NEW:
        assert re.search(rf"^\s*(?:size_t|int)\s+{f}\s*\(", text, re.M), f
        assert f in native.TRAIN_EXPORTS
    assert int(re.search(r"#define GSR_EXPOSURE_CLAMP (\d+)u?", text).group(1)) == native.EXPOSURE_CLAMP == 1
    out = subprocess.run(["nm", "-D", "--defined-only", native.hip_library_path()], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW if f not in syms]
    assert native.load_hip().gsr_abi_version() == native.ABI_VERSION == 4  # new symbols only


def test_scratch_bytes_positive_monotone_and_bounded():
    L = pkg("native").load_hip()
    shapes = [(1, 1), (1, 3), (16, 16), (70, 101), (33, 200), (480, 640), (1080, 1920), (1024, 2049), (2160, 3840),
              (8192, 8192)]
    shapes.sort(key=lambda s: s[0] * s[1])
    sizes = [int(L.gsr_exposure_scratch_bytes(h, w)) for h, w in shapes]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] < sizes[-1]
    # one 48-byte partial (12 floats) per block; the grid is capped at 2048 blocks, so the scratch is too
    assert sizes[-1] <= 2048 * 48 + 256


def test_validation_without_gpu():
    native = pkg("native")
    L = native.load_hip()
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first

    def fwd(img=fake, exposure=fake, H=8, W=8, flags=0, out=fake):
        return L.gsr_exposure_forward(img, exposure, H, W, flags, out, None)

    def bwd(img=fake, exposure=fake, dout=fake, H=8, W=8, flags=0, scratch=fake, dimg=fake, dexp=fake):
        return L.gsr_exposure_backward(img, exposure, dout, H, W, flags, scratch, dimg, dexp, None)

    shapes = [dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)]
    flags = [dict(flags=2), dict(flags=3), dict(flags=1 << 31)]
    bad_fwd = shapes + flags + [dict(img=None), dict(exposure=None), dict(out=None)]
    bad_bwd = shapes + flags + [dict(img=None), dict(exposure=None), dict(dout=None), dict(scratch=None),
                                dict(dimg=None), dict(dexp=None)]
    for call, bad in ((fwd, bad_fwd), (bwd, bad_bwd)):
        for kw in bad:
            assert call(**kw) < 0, (call.__name__, kw)
            assert "exposure" in native.last_error(), (kw, native.last_error())


def test_exposures_round_trip_and_upstream_layout(tmp_path):
    sio = pkg("scene_io")
    rng = np.random.default_rng(0)
    e = (np.eye(3, 4)[None] + 0.1 * rng.standard_normal((4, 3, 4))).astype(np.float32)
    e[0, 0, 0] = np.float32(1.0) / np.float32(3.0)          # not representable in few decimal digits
    e[1, 2, 3] = np.nextafter(np.float32(0.0), np.float32(1.0))  # a subnormal
    names = ["DSC_0001", "DSC_0002", "img 3", "4"]
    path = tmp_path / "exposure.json"
    sio.save_exposures(str(path), names, e)
    raw = json.loads(path.read_text())
    assert list(raw) == names and all(np.asarray(raw[n]).shape == (3, 4) for n in names)
    back = sio.load_exposures(str(path))
    assert list(back) == names
    for i, n in enumerate(names):
        assert back[n].dtype == np.float32 and back[n].shape == (3, 4)
        assert back[n].tobytes() == e[i].tobytes(), n  # bit-exact
    with pytest.raises(ValueError):
        sio.save_exposures(str(path), names[:3], e)
    # a literal in upstream's layout (exposure.json as train.py writes it)
    literal = """{
  "DSCF4667": [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
  "DSCF4668": [[0.9538, 0.0123, -0.004, 0.0213], [-0.0071, 1.0312, 0.0009, -0.0154], [0.002, -0.0135, 1.087, 0.0068]]
}"""
    lit = tmp_path / "upstream.json"
    lit.write_text(literal)
    got = sio.load_exposures(str(lit))
    assert list(got) == ["DSCF4667", "DSCF4668"]
    np.testing.assert_array_equal(got["DSCF4667"], np.eye(3, 4, dtype=np.float32))
    np.testing.assert_array_equal(got["DSCF4668"], np.array(
        [[0.9538, 0.0123, -0.004, 0.0213], [-0.0071, 1.0312, 0.0009, -0.0154], [0.002, -0.0135, 1.087, 0.0068]],
        np.float64).astype(np.float32))
    bad = tmp_path / "bad.json"
    bad.write_text('{"a": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]}')
    with pytest.raises(ValueError):
        sio.load_exposures(str(bad))


def test_optimization_params_and_schedule():
    T, general = pkg("trainer"), pkg("general")
    o = T.OptimizationParams()
    assert o.train_exposure is False and o.exposure_clamp is True
    assert (o.exposure_lr_init, o.exposure_lr_final) == (0.01, 0.001)
    assert (o.exposure_lr_delay_steps, o.exposure_lr_delay_mult) == (0, 0.0)
    f = general.get_expon_lr_func(o.exposure_lr_init, o.exposure_lr_final, lr_delay_steps=o.exposure_lr_delay_steps,
                                  lr_delay_mult=o.exposure_lr_delay_mult, max_steps=o.iterations)
    assert math.isclose(f(0), 0.01, rel_tol=1e-12)
    assert math.isclose(f(o.iterations), 0.001, rel_tol=1e-12)
    assert general.get_expon_lr_func(0.0, 0.0, max_steps=o.iterations)(5) == 0.0  # both 0: a frozen exposure


def test_write_scene_refuses_train_exposure(tmp_path):
    L, T = pkg("train_loop"), pkg("trainer")
    scene = L.LoopScene(cams=[], gts=[], points=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32),
                        extent=1.0)
    with pytest.raises(ValueError, match="exposure"):
        L.write_scene(str(tmp_path / "scene.bin"), scene, 10, opt=T.OptimizationParams(train_exposure=True))
