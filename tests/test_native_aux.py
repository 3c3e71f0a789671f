"""Depth and alpha outputs (gsr_forward_aux / gsr_backward_aux): the reference the GPU tests use, pinned
on the CPU, and the ABI checks that need no GPU.

The reference is the unchanged CPU oracle composed twice (`aux_reference`): a colour render, then a
render of the same geometry with colors_precomp = (v, 1, 0) per Gaussian (v = the view-space depth
z, or 1 / z) over a black background, whose red channel is the expected depth and whose green
channel is the expected alpha.  Gradients add up, plus the one path the second render cannot see:
v depends on the mean through z, dL/dmeans3D += dL/dz * (V[2], V[6], V[10]).
`test_aux_reference_vs_fp64` holds that composition against the independent fp64 autograd
restatement (tests/golden/dense_reference.py rendered twice in one graph, the second render's
colours built from the differentiable view-space depth).
"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg, rel_l2

HEADER = os.path.join(ROOT, "include", "gsr", "gsr.h")
SUMMED = ["means2D", "conic", "opacities", "scales", "rotations", "cov3D"]  # g1 + g2
COLOUR_ONLY = ["sh_dc", "sh_rest", "colors"]                                 # g1 alone


def aux_reference(oracle, cam, inputs, sh_degree, dL_dcolor, dL_ddepth=None, dL_dalpha=None, inverse=False,
                  bg=(0.0, 0.0, 0.0), scale_modifier=1.0):
    """Expected outputs and gradients of forward_aux / backward_aux from the oracle.  `inputs`: the
    forward's keyword inputs (means3D, opacities, scales / rotations or cov3D_precomp, sh_dc / sh_rest
    or colors_precomp) as host arrays.  Returns dict(color, depth, alpha, radii, num_rendered,
    grads, f1) -- f1 is the colour render's OracleForward (sorted list, ranges, ...)."""
    g = inputs.get
    geom = dict(scales=g("scales"), rotations=g("rotations"), cov3D_precomp=g("cov3D_precomp"),
                scale_modifier=scale_modifier)
    f1 = oracle.forward(cam, g("means3D"), g("opacities"), sh_dc=g("sh_dc"), sh_rest=g("sh_rest"),
                        sh_degree=sh_degree, colors_precomp=g("colors_precomp"), bg=bg, **geom)
    H, W = cam.height, cam.width
    zero = np.zeros((H, W), np.float32)
    dD = zero if dL_ddepth is None else np.asarray(dL_ddepth, np.float32).reshape(H, W)
    dA = zero if dL_dalpha is None else np.asarray(dL_dalpha, np.float32).reshape(H, W)
    g1 = f1.state.backward(np.asarray(dL_dcolor, np.float32).reshape(3, H, W))
    z = f1.state.preprocess()["depth"].astype(np.float32)
    vis = f1.radii > 0
    one = np.float32(1.0)
    zs = np.where(vis, z, one)  # culled Gaussians blend nothing: keep 1 / z finite there
    v = (one / zs) if inverse else zs
    aux = np.stack([v, np.ones_like(v), np.zeros_like(v)], 1).astype(np.float32)
    aux[~vis] = 0.0
    f2 = oracle.forward(cam, g("means3D"), g("opacities"), colors_precomp=aux, sh_degree=0, bg=(0.0, 0.0, 0.0),
                        **geom)
    assert f2.num_rendered == f1.num_rendered and np.array_equal(f2.radii, f1.radii)
    g2 = f2.state.backward(np.stack([dD, dA, zero]))
    grads = {}
    for k in SUMMED:
        grads[k] = g1[k] + g2[k]
    for k in COLOUR_ONLY:
        grads[k] = g1[k]
    dz = g2["colors"][:, 0].astype(np.float64)
    if inverse:
        dz = -dz / zs.astype(np.float64) ** 2
    V = np.asarray(cam.viewmatrix, np.float64)
    grads["means3D"] = (g1["means3D"].astype(np.float64) + g2["means3D"] +
                        dz[:, None] * np.array([V[2], V[6], V[10]])[None, :]).astype(np.float32)
    grads["dz_term"] = (dz[:, None] * np.array([V[2], V[6], V[10]])[None, :]).astype(np.float32)
    return dict(color=f1.color, depth=f2.color[0].copy(), alpha=f2.color[1].copy(), radii=f1.radii,
                num_rendered=f1.num_rendered, grads=grads, f1=f1, z=z)


def make_aux_grads(cam, seed):
    """Random dL/ddepth and dL/dalpha images (H x W, in [-1, 1))."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (cam.height, cam.width)).astype(np.float32),
            rng.uniform(-1.0, 1.0, (cam.height, cam.width)).astype(np.float32))


@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "invdepth"])
def test_aux_reference_vs_fp64(inverse, oracle):
    """256 Gaussians / 64x48 / SH3 (the sh3_64x48 fixture's scene): the oracle composition against
    fp64 autograd of the dense restatement rendered twice in one graph.  rel-L2 <= 2e-5 per tensor,
    the bar test_oracle_matches_golden holds the oracle to."""
    import torch
    import dense_reference as dref
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(64, 48)
    s = sc.make_scene(cam, 256, max_sh_degree=3, seed=0)
    dC = sc.make_dL_dpix(cam, seed=1)
    dD, dA = make_aux_grads(cam, seed=2)
    inputs = dict(means3D=s.means3D, opacities=s.opacities, scales=s.scales, rotations=s.rotations, sh_dc=s.sh_dc,
                  sh_rest=s.sh_rest)
    ref = aux_reference(oracle, cam, inputs, 3, dC, dD, dA, inverse=inverse)

    dt = torch.float64
    leaf = lambda a: torch.tensor(np.asarray(a), dtype=dt, requires_grad=True)
    L = {k: leaf(v) for k, v in inputs.items()}
    pre = dref.preprocess(cam, L["means3D"], L["opacities"], scales=L["scales"], rots=L["rotations"],
                          sh_dc=L["sh_dc"], sh_rest=L["sh_rest"], D=3, dtype=dt)
    geom = dref.geometry_f32(cam, s.means3D, s.opacities, scales=s.scales, rots=s.rotations)
    np.testing.assert_array_equal(geom["radius"].numpy(), ref["radii"])
    color, _, _ = dref.render(cam, pre, geom, (0.0, 0.0, 0.0))
    tz = pre["tz"]
    v = 1.0 / tz if inverse else tz
    pre2 = dict(pre)
    pre2["rgb"] = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1)
    aux, T, _ = dref.render(cam, pre2, geom, (0.0, 0.0, 0.0))
    loss = (color * torch.tensor(dC, dtype=dt)).sum() + (aux[0] * torch.tensor(dD, dtype=dt)).sum() + \
        (aux[1] * torch.tensor(dA, dtype=dt)).sum()
    names = list(L)
    grads = torch.autograd.grad(loss, [L[k] for k in names] + [pre["hook"]])
    want = {k: g.numpy() for k, g in zip(names + ["means2D"], grads)}
    assert rel_l2(ref["depth"], aux[0].detach().numpy()) <= 2e-5
    assert rel_l2(ref["alpha"], aux[1].detach().numpy()) <= 2e-5
    assert rel_l2(ref["alpha"], 1.0 - T.detach().numpy()) <= 2e-5  # alpha = 1 - final T
    got = ref["grads"]
    assert rel_l2(got["means2D"][:, :2], want["means2D"]) <= 2e-5
    for k in ("means3D", "opacities", "scales", "rotations", "sh_dc", "sh_rest"):
        r = rel_l2(got[k].reshape(want[k].shape), want[k])
        print(k, r)
        assert r <= 2e-5, (k, r)
    # the dz path is no rounding detail: leaving it out misses the bar by orders of magnitude
    assert rel_l2(got["means3D"] - got["dz_term"], want["means3D"]) > 1e-3


# ---- ABI (no GPU: every check below returns before a device call) ----
def test_aux_symbols_exported_and_declared():
    native = pkg("native")
    new = ["gsr_forward_aux", "gsr_backward_aux", "gsr_binning_bytes_aux", "gsr_image_bytes_aux",
           "gsr_scratch_bytes_aux"]
    assert set(new) <= set(native.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", native.hip_library_path()], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in new if f not in syms]
    text = open(HEADER).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)u?", text).group(1))
    assert val("GSR_ABI_VERSION") == native.ABI_VERSION == native.load_hip().gsr_abi_version() == 4
    assert val("GSR_FLAG_AUX") == native.GSR_FLAG_AUX and val("GSR_FLAG_INVDEPTH") == native.GSR_FLAG_INVDEPTH
    assert val("GSR_LAYOUT_AUX") == native.GSR_LAYOUT_AUX and val("GSR_LAYOUT_INVDEPTH") == native.GSR_LAYOUT_INVDEPTH
    # the new bits are free: no other flag / layout bit shares them
    assert native.GSR_FLAG_AUX & (native.GSR_FLAG_DEBUG | native.GSR_FLAG_ROW_SPANS) == 0
    assert native.GSR_FLAG_INVDEPTH & (native.GSR_FLAG_DEBUG | native.GSR_FLAG_ROW_SPANS | native.GSR_FLAG_AUX) == 0
    assert (native.GSR_LAYOUT_AUX | native.GSR_LAYOUT_INVDEPTH) & (val("GSR_LAYOUT_ROW_BUCKETED") |
                                                                    val("GSR_LAYOUT_PRESORT")) == 0


def test_aux_structs_match_the_c_layout():
    native = pkg("native")
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "gsr/gsr.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(gsr_aux_out), sizeof(gsr_aux_grads), offsetof(gsr_aux_out, alpha),
         offsetof(gsr_aux_grads, dL_dalpha));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sz = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [ctypes.sizeof(native.AuxOut), ctypes.sizeof(native.AuxGrads), native.AuxOut.alpha.offset,
            native.AuxGrads.dL_dalpha.offset] == sz
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = re.search(r"```python\n(# ctypes binding stub.*?)```", text, re.S)
    ns = {}
    exec(stub.group(1), ns)
    for name, mine in (("AuxOut", native.AuxOut), ("AuxGrads", native.AuxGrads)):
        assert ctypes.sizeof(ns[name]) == ctypes.sizeof(mine), name
        assert [f[0] for f in ns[name]._fields_] == [f[0] for f in mine._fields_], name


def test_aux_size_queries():
    """The aux buffers are the plain ones plus: one H x W plane (image), 1 KB per checkpoint slot
    (binning), 4 B per entry (scratch).  The plain queries return what they always did."""
    L = pkg("native").load_hip()
    up = lambda n: (n + 255) // 256 * 256
    assert L.gsr_image_bytes_aux(1920, 1080) == L.gsr_image_bytes(1920, 1080) + up(4 * 1920 * 1080)
    slots = L.gsr_ck_pool_slots(7_200_000, 1920, 1080)
    assert L.gsr_binning_bytes_aux(7_200_000, 1920, 1080) == L.gsr_binning_bytes(7_200_000, 1920, 1080) + 1024 * slots
    assert L.gsr_scratch_bytes_aux(1 << 20) == L.gsr_scratch_bytes(1 << 20) + (4 << 20)
    assert L.gsr_scratch_bytes(1 << 20) == (32 << 20) + (4 << 20) + (1 << 20)


def test_aux_validation_without_gpu():
    native = pkg("native")
    L = native.load_hip()
    c = native.Camera()
    c.width, c.height = 64, 48
    g = native.Gaussians()
    g.P, g.sh_degree = 5, 0
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first
    g.means3D = g.opacities = g.sh_dc = g.scales = g.rotations = fake
    s = native.Settings()
    s.tile_y1 = 2**31 - 1
    calls = []
    alloc = native.ALLOC_FN(lambda _c, n: calls.append(n) or 0)
    b = native.Buffers()
    fwd = lambda aux: L.gsr_forward_aux(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), fake, fake, alloc, alloc,
                                        alloc, None, ctypes.byref(b), None, aux)
    # a NULL aux struct, or one without outputs
    assert fwd(None) < 0 and "aux" in native.last_error()
    assert fwd(ctypes.byref(native.AuxOut(None, None))) < 0 and "aux" in native.last_error()
    # a tile band
    ok = native.AuxOut(fake.value, fake.value)
    s.tile_y0, s.tile_y1 = 1, 2
    assert fwd(ctypes.byref(ok)) < 0 and "full images only" in native.last_error()
    gr = native.Grads()
    gr.dL_dmeans2D = gr.dL_dopacity = gr.dL_dmeans3D = gr.dL_dsh_dc = gr.dL_dscales = gr.dL_drotations = fake
    ag = native.AuxGrads(None, None)

    def bwd(layout, flags=0, aux=ag, capacity=64):
        bb = native.Buffers()
        bb.geom = bb.binning = bb.image = fake
        bb.n_local, bb.capacity, bb.num_rendered, bb.layout = 5, capacity, capacity, layout
        s.flags = flags
        return L.gsr_backward_aux(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), ctypes.byref(bb), fake, alloc,
                                  None, ctypes.byref(gr), None, ctypes.byref(aux) if aux is not None else None)

    text = open(HEADER).read()
    hexval = lambda name: int(re.search(rf"#define {name} (0x[0-9A-Fa-f]+|\d+)u?", text).group(1), 0)
    TAG, RB, AUX, INV = (hexval("GSR_LAYOUT_" + n) for n in ("TAG", "ROW_BUCKETED", "AUX", "INVDEPTH"))
    assert bwd(TAG | RB | AUX) < 0 and "full images only" in native.last_error()  # still the band
    s.tile_y0, s.tile_y1 = 0, 2**31 - 1
    assert bwd(TAG | RB | AUX, aux=None) < 0 and "aux" in native.last_error()
    # plain buffers (a gsr_forward's layout word): refused, GSR_ERR_LAYOUT
    assert bwd(TAG | RB) == native.GSR_ERR_LAYOUT and "GSR_LAYOUT_AUX" in native.last_error()
    assert bwd(0) == native.GSR_ERR_LAYOUT
    # the forward's depth mode must match the settings'
    assert bwd(TAG | RB | AUX, flags=native.GSR_FLAG_INVDEPTH) == native.GSR_ERR_LAYOUT
    assert "INVDEPTH" in native.last_error()
    assert bwd(TAG | RB | AUX | INV, flags=0) == native.GSR_ERR_LAYOUT
    assert bwd(TAG | RB | INV) == native.GSR_ERR_LAYOUT  # INVDEPTH without AUX is no forward's word
    assert calls == [], "nothing may be allocated before the checks"
