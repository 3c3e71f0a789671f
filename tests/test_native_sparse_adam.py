"""The visibility-masked Adam step (gsr_adam_step_sparse, include/gsr/gsr_train.h) without a GPU:
the entry point is declared, listed and exported; every refusal comes back < 0 with "adam" in the
error text before any device call (the pointers below are fake and never dereferenced); the
nothing-to-do cases return 0; and the trainer's switch has its default and refuses unknown values."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, pkg

TRAIN_HEADER = os.path.join(ROOT, "include", "gsr", "gsr_train.h")
FAKE = 4096           # 16-byte aligned, never dereferenced
RADII = ctypes.c_void_p(8192)
P = 10


def _groups(native, count=1, **over):
    g = (native.AdamGroup * max(count, 1))()
    for i in range(count):
        g[i].param = g[i].grad = g[i].exp_avg = g[i].exp_avg_sq = FAKE
        g[i].n, g[i].act, g[i].step, g[i].lr = 3 * P, native.ACT_NONE, 1, 1e-3
        for k, v in over.items():
            setattr(g[i], k, v)
    return g


def _call(L, g, ngroups, radii=RADII, p=P, guard=None, cap=0):
    return L.gsr_adam_step_sparse(g, ngroups, radii, p, 0.9, 0.999, 1e-8, guard, cap, None)


def test_declared_listed_and_exported():
    native = pkg("native")
    text = open(TRAIN_HEADER).read()
    assert re.search(r"^int gsr_adam_step_sparse\(const gsr_adam_group\* groups, int32_t ngroups,\s*"
                     r"const int32_t\* radii, int32_t P,", text, re.M)
    assert "gsr_adam_step_sparse" in native.TRAIN_EXPORTS
    so = native.hip_library_path()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gsr_adam_step_sparse" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = native.load_hip()
    assert L.gsr_adam_step_sparse.restype is ctypes.c_int and len(L.gsr_adam_step_sparse.argtypes) == 10


REFUSALS = {
    "null radii": lambda n: dict(g=_groups(n), radii=None),
    "negative P": lambda n: dict(g=_groups(n), p=-1),
    "n no multiple of P": lambda n: dict(g=_groups(n, n=3 * P + 1)),
    "normalize width 6": lambda n: dict(g=_groups(n, n=6 * P, act=n.ACT_NORMALIZE4)),
    "normalize n % 4": lambda n: dict(g=_groups(n, n=3 * P, act=n.ACT_NORMALIZE4)),
    "negative group count": lambda n: dict(g=_groups(n), ngroups=-1),
    "nine groups": lambda n: dict(g=_groups(n, 9), ngroups=9),
    "null groups": lambda n: dict(g=None),
    "negative n": lambda n: dict(g=_groups(n, n=-3 * P)),
    "null param": lambda n: dict(g=_groups(n, param=None)),
    "null grad": lambda n: dict(g=_groups(n, grad=None)),
    "null exp_avg": lambda n: dict(g=_groups(n, exp_avg=None)),
    "null exp_avg_sq": lambda n: dict(g=_groups(n, exp_avg_sq=None)),
    "step 0": lambda n: dict(g=_groups(n, step=0)),
    "activation -1": lambda n: dict(g=_groups(n, act=-1)),
    "activation 4": lambda n: dict(g=_groups(n, act=4)),
    "param off 16 bytes": lambda n: dict(g=_groups(n, param=FAKE + 4)),
    "grad off 16 bytes": lambda n: dict(g=_groups(n, grad=FAKE + 8)),
    "moment off 16 bytes": lambda n: dict(g=_groups(n, exp_avg_sq=FAKE + 12)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_without_gpu(case):
    native = pkg("native")
    L = native.load_hip()
    kw = REFUSALS[case](native)
    kw.setdefault("ngroups", 1)
    g = kw.pop("g")
    ngroups = kw.pop("ngroups")
    assert _call(L, g, ngroups, **kw) < 0, case
    assert "adam" in native.last_error(), (case, native.last_error())


def test_the_second_group_is_checked_too():
    native = pkg("native")
    L = native.load_hip()
    g = _groups(native, 2)
    g[1].n = 45 * P + 5
    assert _call(L, g, 2) < 0 and "adam" in native.last_error()


def test_nothing_to_do_returns_zero():
    native = pkg("native")
    L = native.load_hip()
    assert _call(L, _groups(native), 0) == 0
    assert _call(L, None, 0, radii=None, p=0) == 0
    assert _call(L, _groups(native), 1, p=0) == 0
    assert _call(L, _groups(native), 1, radii=None, p=0) == 0
    # only empty groups (f_rest at SH degree 0): no launch either
    assert _call(L, _groups(native, n=0), 1) == 0


def test_optimizer_type_default_and_refusal():
    trainer = pkg("trainer")
    assert trainer.OptimizationParams().optimizer_type == "default"
    assert trainer.OptimizationParams(optimizer_type="sparse_adam").optimizer_type == "sparse_adam"
    tr = object.__new__(trainer.GaussianTrainer)  # setup() refuses before it touches any state
    with pytest.raises(ValueError, match="optimizer_type"):
        tr.setup(trainer.OptimizationParams(optimizer_type="adamw"))
