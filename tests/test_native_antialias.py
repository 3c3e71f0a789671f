"""Anti-aliased rendering (GSR_FLAG_ANTIALIAS): the reference the GPU tests use, pinned on the CPU, and
the ABI checks that need no GPU.

The flag multiplies every opacity by coef = sqrt(max(0.000025, det0 / det1)), det0 and det1 the
determinants of the EWA 2D covariance before and after the 0.3 px^2 dilation, and changes nothing
else.  So the reference is a composition of the unchanged CPU oracle: run it on opacities o' = o coef
(`coef_f32`: coef restated in f32 in the kernel's operation order, plus its fp64 value), then carry
its gradients to the leaves (`apply_aa_chain`): dL/do = coef dL/do', and the covariance and mean
leaves gain the fp64 autograd gradient of sum_g coef_g o_g dL/do'_g.
`test_composition_vs_fp64` holds that composition against the independent fp64 autograd restatement
(tests/golden/dense_reference.py) rendered with opacity * coef in the graph.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg, rel_l2

HEADER = os.path.join(ROOT, "include", "gsr", "gsr.h")
H_DIL = 0.3          # the dilation, px^2
R_CLAMP = 0.000025   # the floor of det0 / det1
GEOM_LEAVES = ("means3D", "scales", "rotations", "cov3D")


class _Np32:
    """numpy float32: every +, -, *, /, sqrt is one correctly rounded IEEE operation, as F1's are.
    (torch's CPU float32 sqrt / divide are not on every machine: its coef missed the GPU's and this
    one's, which agree on every Gaussian, by one ulp in 0.6 % to 18 % of a scene.)"""
    const = staticmethod(np.float32)
    minimum, maximum, sqrt, where = (staticmethod(f) for f in (np.minimum, np.maximum, np.sqrt, np.where))


class _T64:
    """torch float64: the differentiable restatement."""
    @staticmethod
    def const(v):
        import torch
        return torch.tensor(float(np.float32(v)), dtype=torch.float64)

    @staticmethod
    def _t(name):
        import torch
        return getattr(torch, name)

    minimum = staticmethod(lambda a, b: _T64._t("minimum")(a, b))
    maximum = staticmethod(lambda a, b: _T64._t("maximum")(a, b))
    sqrt = staticmethod(lambda a: _T64._t("sqrt")(a))
    where = staticmethod(lambda c, a, b: _T64._t("where")(c, a, b))


def _cov2d(cam, means, scales, rots, cov3D, scale_mod, xp):
    """(a0, b, c0): the EWA 2D covariance before the dilation, in F1's operation order
    (gsr_preprocess.hip preprocess_geom) -- with xp = _Np32 every value is F1's bit for bit; with
    _T64 and leaf tensors it is the differentiable restatement."""
    k = xp.const  # camera values are f32
    V = [k(v) for v in cam.viewmatrix]
    x, y, z = means[:, 0], means[:, 1], means[:, 2]
    tx = V[0] * x + V[4] * y + V[8] * z + V[12]
    ty = V[1] * x + V[5] * y + V[9] * z + V[13]
    tz = V[2] * x + V[6] * y + V[10] * z + V[14]
    one, two = k(1.0), k(2.0)
    if cov3D is None:
        r, qx, qy, qz = rots[:, 0], rots[:, 1], rots[:, 2], rots[:, 3]
        R = [one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy),
             two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx),
             two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]
        s = [k(scale_mod) * scales[:, j] for j in range(3)]
        L = [R[3 * i + j] * s[j] for i in range(3) for j in range(3)]
        sig = lambda i, j: L[3 * i] * L[3 * j] + L[3 * i + 1] * L[3 * j + 1] + L[3 * i + 2] * L[3 * j + 2]
        c3 = [sig(0, 0), sig(0, 1), sig(0, 2), sig(1, 1), sig(1, 2), sig(2, 2)]
    else:
        c3 = [cov3D[:, j] for j in range(6)]
    Wf, Hf = k(cam.width), k(cam.height)
    tfx, tfy = k(cam.tanfovx), k(cam.tanfovy)
    fx, fy = Wf / (two * tfx), Hf / (two * tfy)
    limx, limy = k(1.3) * tfx, k(1.3) * tfy
    cx = xp.minimum(limx, xp.maximum(-limx, tx / tz)) * tz
    cy = xp.minimum(limy, xp.maximum(-limy, ty / tz)) * tz
    tz2 = tz * tz
    J00, J02 = fx / tz, -(fx * cx) / tz2
    J11, J12 = fy / tz, -(fy * cy) / tz2
    T0 = [J00 * V[4 * i + 0] + J02 * V[4 * i + 2] for i in range(3)]
    T1 = [J11 * V[4 * i + 1] + J12 * V[4 * i + 2] for i in range(3)]
    S = [c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]]
    U0 = [T0[0] * S[j] + T0[1] * S[3 + j] + T0[2] * S[6 + j] for j in range(3)]
    U1 = [T1[0] * S[j] + T1[1] * S[3 + j] + T1[2] * S[6 + j] for j in range(3)]
    a0 = U0[0] * T0[0] + U0[1] * T0[1] + U0[2] * T0[2]
    b = U0[0] * T1[0] + U0[1] * T1[1] + U0[2] * T1[2]
    c0 = U1[0] * T1[0] + U1[1] * T1[1] + U1[2] * T1[2]
    return a0, b, c0


def _coef(cam, means, scales, rots, cov3D, scale_mod, xp):
    """coef = sqrt(max(0.000025, det0 / det1)) in the kernel's order; the clamp passes no gradient
    (r <= 0.000025 -> 0, upstream's rule)."""
    a0, b, c0 = _cov2d(cam, means, scales, rots, cov3D, scale_mod, xp)
    h = xp.const(H_DIL)
    a, c = a0 + h, c0 + h
    det = a * c - b * b
    r = (a0 * c0 - b * b) / det
    lo = xp.const(R_CLAMP)
    return xp.sqrt(xp.where(r > lo, r, lo)), r


LEAF_KEYS = (("means3D", "means3D"), ("scales", "scales"), ("rotations", "rotations"), ("cov3D", "cov3D_precomp"))


def _leaves(inputs, requires_grad=False):
    """The geometry inputs as float64 torch tensors."""
    import torch
    return {name: None if inputs.get(key) is None else
            torch.tensor(np.asarray(inputs[key], np.float64), dtype=torch.float64, requires_grad=requires_grad)
            for name, key in LEAF_KEYS}


def coef_f32(cam, inputs, scale_modifier=1.0):
    """(coef as F1 computes it in f32, coef in fp64, r in fp64) for every Gaussian of `inputs` (the
    forward's keyword inputs as host arrays).  Values of culled Gaussians are meaningless."""
    import torch
    A = {name: None if inputs.get(key) is None else np.ascontiguousarray(inputs[key], np.float32)
         for name, key in LEAF_KEYS}
    with np.errstate(all="ignore"):  # culled Gaussians (behind the camera, tz = 0) may divide by zero
        c32, _ = _coef(cam, A["means3D"].reshape(-1, 3), A["scales"], A["rotations"], A["cov3D"], scale_modifier, _Np32)
    assert c32.dtype == np.float32
    with torch.no_grad():
        L = _leaves(inputs)
        c64, r64 = _coef(cam, L["means3D"], L["scales"], L["rotations"], L["cov3D"], scale_modifier, _T64)
    return c32, c64.numpy(), r64.numpy()


def compensated(opacities, coef32):
    """o' as F1 stores it: the f32 product."""
    return (np.asarray(opacities, np.float32).reshape(-1) * np.asarray(coef32, np.float32)).astype(np.float32)


def apply_aa_chain(cam, inputs, grads, scale_modifier=1.0, chain=True):
    """Gradients for the leaves from an oracle run on opacities = o' (`grads`, whose "opacities" is
    dL/do').  dL/do = coef dL/do'; means3D and scales / rotations | cov3D gain the fp64 autograd
    gradient of sum_g coef_g o_g dL/do'_g.  chain=False leaves that second term out."""
    import torch
    dt = torch.float64
    L = _leaves(inputs, requires_grad=True)
    co, _ = _coef(cam, L["means3D"], L["scales"], L["rotations"], L["cov3D"], scale_modifier, _T64)
    dop = np.asarray(grads["opacities"], np.float64).reshape(-1)
    o = np.asarray(inputs["opacities"], np.float64).reshape(-1)
    out = {k: np.array(v, copy=True) for k, v in grads.items()}
    out["opacities"] = (co.detach().numpy() * dop).astype(np.float32).reshape(np.shape(grads["opacities"]))
    if chain:
        w = torch.tensor(o * dop, dtype=dt)
        # a culled Gaussian blends nothing (dL/do' = 0): keep its (possibly non-finite) coef out of the sum
        total = torch.where(w != 0, co * w, torch.zeros_like(w)).sum()
        names = [k for k in GEOM_LEAVES if L[k] is not None]
        for k, g in zip(names, torch.autograd.grad(total, [L[k] for k in names])):
            g = torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0).numpy()
            out[k] = (np.asarray(grads[k], np.float64) + g.reshape(np.shape(grads[k]))).astype(np.float32)
    return out


def aa_scene(cam, P, seed=0):
    """make_scene with every second Gaussian a tenth of its size and every sixteenth (from 3) a
    thousandth: sub-pixel footprints, some at the clamp."""
    s = pkg("scene").make_scene(cam, P, max_sh_degree=3, seed=seed)
    s.scales[::2] *= 0.1
    s.scales[3::16] *= 1e-3
    s.raw_scales = np.log(s.scales.astype(np.float64)).astype(np.float32)  # the raw leaves follow the edit
    return s


def scene_inputs(s):
    return dict(means3D=s.means3D, opacities=s.opacities, scales=s.scales, rotations=s.rotations, sh_dc=s.sh_dc,
                sh_rest=s.sh_rest)


def aa_oracle(oracle, cam, inputs, sh_degree, dL_dcolor, o_prime=None, bg=(0.0, 0.0, 0.0), scale_modifier=1.0,
              chain=True):
    """The flagged forward / backward from the oracle: run on o' (given -- e.g. the GPU's own -- or
    f32(o coef_f32)), gradients through apply_aa_chain.  Returns (OracleForward, grads, o')."""
    g = inputs.get
    if o_prime is None:
        o_prime = compensated(g("opacities"), coef_f32(cam, inputs, scale_modifier)[0])
    f = oracle.forward(cam, g("means3D"), o_prime, scales=g("scales"), rotations=g("rotations"), sh_dc=g("sh_dc"),
                       sh_rest=g("sh_rest"), sh_degree=sh_degree, colors_precomp=g("colors_precomp"),
                       cov3D_precomp=g("cov3D_precomp"), scale_modifier=scale_modifier, bg=bg)
    raw = f.state.backward(np.asarray(dL_dcolor, np.float32).reshape(3, cam.height, cam.width))
    return f, apply_aa_chain(cam, inputs, raw, scale_modifier, chain=chain), o_prime


def test_composition_vs_fp64(oracle):
    """256 Gaussians / 64x48 / SH3, the scale-edited scene: the oracle on o' plus the chain against fp64
    autograd of the dense restatement with opacity * coef in the graph.  rel-L2 <= 2e-5 per tensor
    (test_oracle_matches_golden's bar); without the chain term `scales` is off by more than 1e-3."""
    import torch
    import dense_reference as dref
    cam = pkg("graphics").synthetic_camera(64, 48)
    s = aa_scene(cam, 256)
    inputs = scene_inputs(s)
    dC = pkg("scene").make_dL_dpix(cam, seed=1)
    f, got, _ = aa_oracle(oracle, cam, inputs, 3, dC)
    _, nochain, _ = aa_oracle(oracle, cam, inputs, 3, dC, chain=False)

    dt = torch.float64
    L = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in inputs.items()}
    pre = dref.preprocess(cam, L["means3D"], L["opacities"], scales=L["scales"], rots=L["rotations"],
                          sh_dc=L["sh_dc"], sh_rest=L["sh_rest"], D=3, dtype=dt)
    geom = dref.geometry_f32(cam, s.means3D, s.opacities, scales=s.scales, rots=s.rotations)
    np.testing.assert_array_equal(geom["radius"].numpy(), f.radii)
    co, r = _coef(cam, L["means3D"], L["scales"], L["rotations"], None, 1.0, _T64)
    vis = geom["visible"].numpy()
    pre["opacity"] = pre["opacity"] * torch.where(geom["visible"], co, torch.ones_like(co))
    color, _, _ = dref.render(cam, pre, geom, (0.0, 0.0, 0.0))
    # the scene exercises what it is for: sub-pixel footprints, some at the clamp, a visibly different image
    rv = r.detach().numpy()[vis]
    assert (rv <= R_CLAMP).sum() >= 8 and (np.sqrt(np.maximum(rv, R_CLAMP)) < 0.5).mean() > 0.3
    plain = oracle.forward(cam, s.means3D, s.opacities, scales=s.scales, rotations=s.rotations, sh_dc=s.sh_dc,
                           sh_rest=s.sh_rest, sh_degree=3)
    assert rel_l2(f.color, plain.color) > 0.01
    rc = rel_l2(f.color, color.detach().numpy())
    print("color", rc)
    assert rc <= 2e-5
    names = list(L)
    grads = torch.autograd.grad((color * torch.tensor(dC, dtype=dt)).sum(), [L[k] for k in names] + [pre["hook"]])
    want = {k: g.numpy() for k, g in zip(names + ["means2D"], grads)}
    assert rel_l2(got["means2D"][:, :2], want["means2D"]) <= 2e-5
    for k in ("means3D", "opacities", "scales", "rotations", "sh_dc", "sh_rest"):
        e = rel_l2(got[k].reshape(want[k].shape), want[k])
        print(k, e, rel_l2(nochain[k].reshape(want[k].shape), want[k]))
        assert e <= 2e-5, (k, e)
    assert rel_l2(nochain["scales"], want["scales"]) > 1e-3


@pytest.mark.parametrize("P,W,H", [(256, 64, 48), (5000, 300, 200)])
def test_coef_f32_vs_fp64(P, W, H):
    """The f32 restatement of coef is within 1e-5 relative of fp64 on every visible Gaussian."""
    import dense_reference as dref
    cam = pkg("graphics").synthetic_camera(W, H)
    s = aa_scene(cam, P)
    c32, c64, _ = coef_f32(cam, scene_inputs(s))
    vis = dref.geometry_f32(cam, s.means3D, s.opacities, scales=s.scales, rots=s.rotations)["visible"].numpy()
    assert vis.sum() > 0.9 * P
    err = np.abs(c32[vis].astype(np.float64) - c64[vis]) / c64[vis]
    print("max rel", err.max())
    assert err.max() <= 1e-5
    assert c32.dtype == np.float32 and (c32[vis] >= np.float32(0.005)).all() and (c32[vis] < 1.0).all()


def closed_form_case(s2, antialiasing, o=0.9, z=5.0):
    """One isotropic Gaussian of 2D variance s2 px^2 at the centre of a 64x64 image, red on black.
    Returns (cam, inputs, expected summed red channel, tolerance): the blended energy is the integral
    of o_eff G - over the alpha >= 1/255 disc, 2 pi sqrt(det1) (o_eff - 1/255); the tolerance is one
    pixel ring at that cut, (2 pi r_cut + 4) / 255."""
    cam = pkg("graphics").synthetic_camera(64, 64)
    fx = cam.width / (2.0 * cam.tanfovx)
    sigma = math.sqrt(s2) * z / fx
    inputs = dict(means3D=np.array([[0.0, 0.0, z]], np.float32), opacities=np.array([o], np.float32),
                  scales=np.full((1, 3), sigma, np.float32), rotations=np.array([[1.0, 0.0, 0.0, 0.0]], np.float32),
                  colors_precomp=np.array([[1.0, 0.0, 0.0]], np.float32))
    det0, det1 = s2 * s2, (s2 + H_DIL) ** 2
    o_eff = o * math.sqrt(max(R_CLAMP, det0 / det1)) if antialiasing else o
    want = 2.0 * math.pi * math.sqrt(det1) * (o_eff - 1.0 / 255.0)
    r_cut = math.sqrt(2.0 * (s2 + H_DIL) * math.log(255.0 * o_eff))
    return cam, inputs, want, (2.0 * math.pi * r_cut + 4.0) / 255.0


CLOSED_FORM = [(s2, aa) for s2 in (0.02, 0.1, 1.0) for aa in (False, True)]


@pytest.mark.parametrize("s2,antialiasing", CLOSED_FORM)
def test_closed_form_energy(s2, antialiasing, oracle):
    cam, inputs, want, tol = closed_form_case(s2, antialiasing)
    op = compensated(inputs["opacities"], coef_f32(cam, inputs)[0]) if antialiasing else inputs["opacities"]
    f = oracle.forward(cam, inputs["means3D"], op, scales=inputs["scales"], rotations=inputs["rotations"],
                       colors_precomp=inputs["colors_precomp"])
    got = float(f.color[0].astype(np.float64).sum())
    print(s2, antialiasing, got, want, tol)
    assert f.color[1:].max() == 0.0
    assert abs(got - want) <= tol
    if antialiasing and s2 == 0.1:  # the compensated sum is the footprint's true energy, 2 pi o sqrt(det0)
        assert abs(got - 2.0 * math.pi * 0.9 * s2) <= tol


# ---- ABI (no GPU: every check below returns before a device call) ----
def _abi_fixture():
    native = pkg("native")
    c = native.Camera()
    c.width, c.height = 64, 48
    g = native.Gaussians()
    g.P, g.sh_degree = 5, 0
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first
    g.means3D = g.opacities = g.sh_dc = g.scales = g.rotations = fake
    s = native.Settings()
    s.tile_y1 = 2**31 - 1
    gr = native.Grads()
    gr.dL_dmeans2D = gr.dL_dopacity = gr.dL_dmeans3D = gr.dL_dsh_dc = gr.dL_dscales = gr.dL_drotations = fake
    return native, native.load_hip(), c, g, s, gr, fake


def test_antialias_constants_and_symbols():
    native = pkg("native")
    text = open(HEADER).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)u?", text).group(1))
    assert val("GSR_FLAG_ANTIALIAS") == native.GSR_FLAG_ANTIALIAS == 16
    assert val("GSR_LAYOUT_ANTIALIAS") == native.GSR_LAYOUT_ANTIALIAS == 16
    assert val("GSR_ABI_VERSION") == native.ABI_VERSION == native.load_hip().gsr_abi_version() == 4
    others = native.GSR_FLAG_DEBUG | native.GSR_FLAG_ROW_SPANS | native.GSR_FLAG_AUX | native.GSR_FLAG_INVDEPTH
    assert native.GSR_FLAG_ANTIALIAS & others == 0
    assert native.GSR_LAYOUT_ANTIALIAS & (val("GSR_LAYOUT_ROW_BUCKETED") | val("GSR_LAYOUT_PRESORT") |
                                          val("GSR_LAYOUT_AUX") | val("GSR_LAYOUT_INVDEPTH")) == 0
    out = subprocess.run(["nm", "-D", "--defined-only", native.hip_library_path()], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in native.EXPORTS if f not in syms]
    rast = pkg("rasterizer")
    assert rast.PipelineParams().antialiasing is False
    assert pkg("trainer").OptimizationParams().antialiasing is False


def test_backward_refuses_flag_layout_disagreement():
    """The backward must run with the forward's GSR_FLAG_ANTIALIAS choice: either disagreement between
    rs->flags and the layout bit is GSR_ERR_LAYOUT, before any allocation or launch."""
    native, L, c, g, s, gr, fake = _abi_fixture()
    text = open(HEADER).read()
    hexval = lambda name: int(re.search(rf"#define {name} (0x[0-9A-Fa-f]+|\d+)u?", text).group(1), 0)
    TAG, RB, AUX, AA = (hexval("GSR_LAYOUT_" + n) for n in ("TAG", "ROW_BUCKETED", "AUX", "ANTIALIAS"))
    calls = []
    alloc = native.ALLOC_FN(lambda _c, n: calls.append(n) or 0)
    V = 2
    cams = (native.Camera * V)(c, c)

    def bufs(layout, n=5):
        b = native.Buffers()
        b.geom = b.binning = b.image = fake
        b.n_local, b.capacity, b.num_rendered, b.layout = n, 64, 64, layout
        return b

    def calls_of(layout):
        b, bv = bufs(layout), bufs(layout, V * 5)
        ag = native.AuxGrads(None, None)
        ba = bufs(layout | AUX)
        return dict(
            gsr_backward=lambda: L.gsr_backward(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), ctypes.byref(b),
                                                fake, alloc, None, ctypes.byref(gr), None),
            gsr_backward_preprocess=lambda: L.gsr_backward_preprocess(ctypes.byref(c), ctypes.byref(g),
                                                                      ctypes.byref(s), ctypes.byref(b), fake,
                                                                      ctypes.byref(gr), None),
            gsr_backward_blend=lambda: L.gsr_backward_blend(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s),
                                                            ctypes.byref(b), fake, alloc, None, fake, None),
            gsr_backward_aux=lambda: L.gsr_backward_aux(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s),
                                                        ctypes.byref(ba), fake, alloc, None, ctypes.byref(gr), None,
                                                        ctypes.byref(ag)),
            gsr_backward_views=lambda: L.gsr_backward_views(V, cams, ctypes.byref(g), ctypes.byref(s),
                                                            ctypes.byref(bv), fake, alloc, None, ctypes.byref(gr),
                                                            None))

    for flag, layout in ((native.GSR_FLAG_ANTIALIAS, TAG | RB), (0, TAG | RB | AA)):
        s.flags = flag
        for name, call in calls_of(layout).items():
            rc = call()
            assert rc == native.GSR_ERR_LAYOUT, (name, flag, rc, native.last_error())
            assert "GSR_FLAG_ANTIALIAS" in native.last_error(), (name, native.last_error())
    # the bit does not disturb the rest of the word's check: a wrong binning choice is still refused
    s.flags = native.GSR_FLAG_ANTIALIAS
    rc = calls_of(TAG | AA)["gsr_backward"]()
    assert rc == native.GSR_ERR_LAYOUT and "disagrees" in native.last_error()
    assert calls == [], "nothing may be allocated before the checks"


def test_shard_and_band_calls_refuse_the_flag():
    """The multi-GPU calls render without the compensation only: the flag is an invalid setting
    (-1), refused before any device call."""
    native, L, c, g, s, gr, fake = _abi_fixture()
    s.flags = native.GSR_FLAG_ANTIALIAS
    s.max_rendered = 64
    rows = (ctypes.c_int32 * 2)(0, 3)
    calls = []
    alloc = native.ALLOC_FN(lambda _c, n: calls.append(n) or 0)
    b = native.Buffers()
    b.geom = b.binning = b.image = fake
    b.n_local, b.capacity = 8, 64
    tried = dict(
        gsr_shard_forward=lambda: L.gsr_shard_forward(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), 1, rows, 8,
                                                      fake, fake, fake, None, None),
        gsr_band_forward=lambda: L.gsr_band_forward(ctypes.byref(c), ctypes.byref(s), 1, 8, fake, fake, alloc, alloc,
                                                    alloc, None, ctypes.byref(b), None),
        gsr_band_backward=lambda: L.gsr_band_backward(ctypes.byref(c), ctypes.byref(s), 1, 8, ctypes.byref(b), fake,
                                                      alloc, None, fake, None),
        gsr_shard_backward=lambda: L.gsr_shard_backward(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), 1, rows, 8,
                                                        fake, fake, ctypes.byref(gr), None))
    for name, call in tried.items():
        rc = call()
        assert rc == -1 and "GSR_FLAG_ANTIALIAS" in native.last_error(), (name, rc, native.last_error())
    assert calls == []
