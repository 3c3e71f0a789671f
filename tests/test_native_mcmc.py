"""The MCMC densification entry points (gsr_mcmc_noise, gsr_mcmc_relocate, include/gsr/gsr_train.h)
without a GPU: both are declared, listed and exported; every refusal comes back < 0 with "mcmc" in the
error text before any device call (the pointers below are fake and never dereferenced); the
nothing-to-do cases return 0; the trainer's switch has its default and refuses unknown values; and the
fp64 reference the GPU tests compare against satisfies its own closed forms."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_reference as ref
from conftest import ROOT, pkg

TRAIN_HEADER = os.path.join(ROOT, "include", "gsr", "gsr_train.h")
FAKE = ctypes.c_void_p(4096)  # 16-byte aligned, never dereferenced
P = 10


def _noise(L, xyz=FAKE, scale=FAKE, rot=FAKE, opac=FAKE, noise=FAKE, p=P, strength=80.0, guard=None, cap=0):
    return L.gsr_mcmc_noise(xyz, scale, rot, opac, noise, p, strength, guard, cap, None)


def _relocate(L, opac=FAKE, scales=FAKE, ratios=FAKE, n=P, min_opacity=0.005, new_o=FAKE, new_s=FAKE):
    return L.gsr_mcmc_relocate(opac, scales, ratios, n, min_opacity, new_o, new_s, None)


def test_declared_listed_and_exported():
    native = pkg("native")
    text = open(TRAIN_HEADER).read()
    assert re.search(r"^int gsr_mcmc_noise\(float\* xyz, const float\* scale_raw, const float\* rot_raw, "
                     r"const float\* opac_raw,\s*const float\* noise, int32_t P, float strength,\s*"
                     r"const uint32_t\* guard_k, uint32_t guard_cap, void\* stream\);", text, re.M)
    assert re.search(r"^int gsr_mcmc_relocate\(const float\* opacities, const float\* scales, const int32_t\* ratios, "
                     r"int32_t n,\s*float min_opacity, float\* new_opacities, float\* new_scales, void\* stream\);",
                     text, re.M)
    assert int(re.search(r"#define GSR_MCMC_MAX_RATIO (\d+)", text).group(1)) == native.MCMC_MAX_RATIO == ref.MAX_RATIO
    so = native.hip_library_path()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = native.load_hip()
    for name, nargs in (("gsr_mcmc_noise", 10), ("gsr_mcmc_relocate", 8)):
        assert name in native.TRAIN_EXPORTS and name in syms
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs


NOISE_REFUSALS = {
    "null xyz": dict(xyz=None),
    "null scales": dict(scale=None),
    "null rotations": dict(rot=None),
    "null opacities": dict(opac=None),
    "null noise": dict(noise=None),
    "negative P": dict(p=-1),
    "negative strength": dict(strength=-1.0),
    "infinite strength": dict(strength=math.inf),
    "nan strength": dict(strength=math.nan),
    "nan strength at P 0": dict(strength=math.nan, p=0),
    "rotations off 16 bytes": dict(rot=ctypes.c_void_p(4096 + 8)),
    "xyz off 4 bytes": dict(xyz=ctypes.c_void_p(4096 + 2)),
    "noise off 4 bytes": dict(noise=ctypes.c_void_p(4096 + 1)),
}

RELOCATE_REFUSALS = {
    "null opacities": dict(opac=None),
    "null scales": dict(scales=None),
    "null ratios": dict(ratios=None),
    "null new opacities": dict(new_o=None),
    "null new scales": dict(new_s=None),
    "negative n": dict(n=-1),
    "min_opacity 0": dict(min_opacity=0.0),
    "min_opacity 1": dict(min_opacity=1.0),
    "min_opacity negative": dict(min_opacity=-0.1),
    "min_opacity nan": dict(min_opacity=math.nan),
}


@pytest.mark.parametrize("case", sorted(NOISE_REFUSALS))
def test_noise_refusals_without_gpu(case):
    native = pkg("native")
    L = native.load_hip()
    assert _noise(L, **NOISE_REFUSALS[case]) < 0, case
    assert "mcmc" in native.last_error(), (case, native.last_error())


@pytest.mark.parametrize("case", sorted(RELOCATE_REFUSALS))
def test_relocate_refusals_without_gpu(case):
    native = pkg("native")
    L = native.load_hip()
    assert _relocate(L, **RELOCATE_REFUSALS[case]) < 0, case
    assert "mcmc" in native.last_error(), (case, native.last_error())


def test_nothing_to_do_returns_zero():
    L = pkg("native").load_hip()
    assert _noise(L, p=0) == 0
    assert _noise(L, xyz=None, scale=None, rot=None, opac=None, noise=None, p=0) == 0
    assert _noise(L, strength=0.0) == 0  # a zero displacement: validated, then no launch
    assert _relocate(L, n=0) == 0
    assert _relocate(L, opac=None, scales=None, ratios=None, new_o=None, new_s=None, n=0) == 0


def test_densify_strategy_default_and_refusal():
    trainer = pkg("trainer")
    opt = trainer.OptimizationParams()
    assert opt.densify_strategy == "default"
    assert (opt.cap_max, opt.noise_lr, opt.opacity_reg, opt.scale_reg, opt.mcmc_min_opacity, opt.mcmc_growth) == \
        (1_000_000, 5e5, 0.01, 0.01, 0.005, 1.05)
    assert trainer.OptimizationParams(densify_strategy="mcmc").densify_strategy == "mcmc"
    tr = object.__new__(trainer.GaussianTrainer)  # setup() refuses before it touches any state
    with pytest.raises(ValueError, match="densify_strategy"):
        tr.setup(trainer.OptimizationParams(densify_strategy="absgrad"))
    with pytest.raises(ValueError, match="mcmc_min_opacity"):
        tr.setup(trainer.OptimizationParams(densify_strategy="mcmc", mcmc_min_opacity=1.0))
    with pytest.raises(ValueError, match="mcmc_growth"):
        tr.setup(trainer.OptimizationParams(densify_strategy="mcmc", mcmc_growth=0.9))


def test_write_scene_refuses_mcmc():
    loop, trainer = pkg("train_loop"), pkg("trainer")
    scene = loop.LoopScene(cams=[], gts=[], points=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32),
                           extent=1.0)
    with pytest.raises(ValueError, match="densif"):
        loop.write_scene(os.devnull, scene, 1, trainer.OptimizationParams(densify_strategy="mcmc"))


# ---------------------------------------------------------------- the reference's own closed forms
def test_reference_ratio_one_is_the_identity():
    for o in (0.005, 0.3, 0.999, ref.OPACITY_MAX):
        x = ref.relocation_x(o, 1)
        assert x == pytest.approx(o, rel=1e-15)
        assert o / ref.relocation_denominator(x, 1) == pytest.approx(1.0, rel=1e-15)
    scales = np.array([[0.5, 0.25, 2.0]], np.float32)
    new_o, new_s = ref.relocate(np.array([0.3], np.float32), scales, [1], 0.005)
    assert new_o[0] == pytest.approx(float(np.float32(0.3)), rel=1e-15)
    assert np.allclose(new_s, scales.astype(np.float64), rtol=1e-15, atol=0.0)


def test_reference_ratio_two_closed_form():
    for o in (0.005, 0.3, 0.999):
        x = ref.relocation_x(o, 2)
        assert x == pytest.approx(1.0 - math.sqrt(1.0 - o), rel=1e-12)
        assert ref.relocation_denominator(x, 2) == pytest.approx(2.0 * x - x * x / math.sqrt(2.0), rel=1e-14)


@pytest.mark.parametrize("n", range(1, ref.MAX_RATIO + 1))
def test_reference_double_sum_equals_the_collapsed_sum(n):
    x = ref.relocation_x(0.5, n)
    a, b = ref.relocation_denominator(x, n), ref.relocation_denominator_collapsed(x, n)
    assert abs(a - b) <= 1e-11 * abs(a), (n, a, b)


def test_reference_ratio_clamp():
    assert [ref.clamp_ratio(v) for v in (0, -3, 1, 51, 52, 1000)] == [1, 1, 1, 51, 51, 51]


def test_reference_gate_vanishes_for_opaque_rows_without_nan():
    o = np.array([0.001, 0.005, 0.5, 0.999])
    g = ref.noise_gate(np.log(o / (1 - o)))
    assert np.isfinite(g).all()
    assert g[0] == pytest.approx(1.0 / (1.0 + math.exp(-0.4)), rel=1e-9) and g[1] == pytest.approx(0.5, rel=1e-9)
    assert 0.0 <= g[3] < g[2] < 1e-20
