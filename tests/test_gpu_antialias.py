"""GPU: anti-aliased rendering (GSR_FLAG_ANTIALIAS) through every surface that takes the flag -- the
C ABI forwards and backwards, views and batch mode, the aux outputs, the autograd Functions, render()
and GaussianTrainer.step -- against the CPU oracle composed as in tests/test_native_antialias.py
(`coef_f32`, `apply_aa_chain`, pinned there against fp64 autograd).

The flag changes F1 and B2 alone, so the shapes are the smallest that reach their variants (SH rows
staged or not, one view or several, with and without the aux channel); image size selects only blend
kernels, which do not change.

Bars (the parity suite's, by value, as in test_gpu_aux.py): images rel-L2 <= 1e-4 and
ELEM_RGB = (1e-4, 1e-3) with at most RGB_FLIPS = 1e-5 outside it; gradients rel-L2 <= 1e-4 and
ELEM_GRAD = (1e-3, 1e-2) with at most GRAD_FLIPS = 1e-3 outside it.  The parity references run on
the GPU's own o', so both sides blend identical opacities.
"""
import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2
from test_native_antialias import (R_CLAMP, aa_oracle, aa_scene, apply_aa_chain, closed_form_case, coef_f32,
                                   compensated, scene_inputs, CLOSED_FORM)
from test_native_aux import aux_reference, make_aux_grads
from test_gpu_parity import elementwise_misses
from test_gpu_views import _cams

import train_oracle as T

pytestmark = pytest.mark.gpu

IMG_REL, GRAD_REL = 1e-4, 1e-4
ELEM_RGB, ELEM_GRAD = (1e-4, 1e-3), (1e-3, 1e-2)
RGB_FLIPS, GRAD_FLIPS = 1e-5, 1e-3
GRAD_KEYS = ["means2D", "conic", "opacities", "means3D", "sh_dc", "sh_rest", "scales", "rotations", "colors",
             "cov3D"]
SEED_MAIN, SEED_PRECOMP = 4, 0  # chosen on the reference alone: see test_parity


@pytest.fixture(scope="module")
def rast():
    return pkg("rasterizer").CAbiRasterizer("cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _records_opacity(st):
    """o' of every Gaussian as F1 stored it: GSR_VIEW_RECORDS slot rec[1].y."""
    native = pkg("native")
    P = st.gauss.P
    rec = _np(st.view(native.VIEW_RECORDS, torch.float32, 12 * P)).reshape(P, 3, 4)
    return rec[:, 1, 1].copy()


def _gpu_o_prime(st, inputs):
    """The GPU's o' for the oracle: the record's value where F1 wrote one, the input opacity elsewhere
    (a Gaussian without a record is culled and blends nothing on either side)."""
    o = np.asarray(inputs["opacities"], np.float32).reshape(-1).copy()
    vis = _np(st.radii) > 0
    o[vis] = _records_opacity(st)[vis]
    return o, vis


def _check_colour(st, f):
    np.testing.assert_array_equal(_np(st.radii), f.radii)
    assert st.num_rendered == f.num_rendered
    a = _np(st.color)
    r = rel_l2(a, f.color)
    frac, worst = elementwise_misses(a, f.color, *ELEM_RGB)
    print(f"colour: rel_l2 {r:.3e} misses {frac:.3e} worst {worst:.3e}")
    assert r <= IMG_REL
    assert frac <= RGB_FLIPS and worst <= 0.01, (frac, worst)


def _check_grads(g_gpu, want_all):
    worst = {}
    for k in GRAD_KEYS:
        if k in g_gpu:
            want = want_all[k]
            a = _np(g_gpu[k]).reshape(want.shape)
            r = rel_l2(a, want)
            worst[k] = elementwise_misses(a, want, *ELEM_GRAD)
            print(f"grad {k}: rel_l2 {r:.3e} misses {worst[k][0]:.3e} |ref| {np.linalg.norm(want):.3e}")
            assert r <= GRAD_REL, (k, r)
    assert max(v[0] for v in worst.values()) <= GRAD_FLIPS, worst


# ---- the main scene: 5000 Gaussians, 300x200, SH3 (F1 with DMA-staged SH rows, B2 with staged rows) ----
@pytest.fixture(scope="module")
def main_case():
    cam = pkg("graphics").synthetic_camera(300, 200)
    s = aa_scene(cam, 5000, seed=SEED_MAIN)
    dC = pkg("scene").make_dL_dpix(cam, seed=2)
    return cam, s, scene_inputs(s), dC


@pytest.fixture(scope="module")
def main_forwards(main_case, rast):
    cam, s, inputs, dC = main_case
    return rast.forward(cam, **inputs, sh_degree=3), rast.forward(cam, **inputs, sh_degree=3, antialiasing=True)


def test_discrete_outputs_unchanged(main_case, main_forwards):
    """1. The flag touches the opacity alone: radii, K, depth keys, tiles touched, the sorted list and
    the ranges are the unflagged call's bit for bit; the colours are not."""
    native = pkg("native")
    cam, s, inputs, dC = main_case
    off, on = main_forwards
    P, tiles = 5000, cam.grid[0] * cam.grid[1]
    K = off.num_rendered
    assert on.num_rendered == K and K > 0
    assert torch.equal(off.radii, on.radii)
    for what, n in ((native.VIEW_DEPTH_KEY, P), (native.VIEW_TILES_TOUCHED, P), (native.VIEW_SORTED_GID, K),
                    (native.VIEW_SORTED_TILE, K), (native.VIEW_RANGES, 2 * tiles)):
        a, b = off.view(what, torch.int32, n), on.view(what, torch.int32, n)
        assert a.numel() == n and torch.equal(a, b), what
    assert not torch.equal(off.color, on.color)
    assert on.buffers.layout == off.buffers.layout | native.GSR_LAYOUT_ANTIALIAS
    assert off.buffers.layout & native.GSR_LAYOUT_ANTIALIAS == 0


def test_compensated_opacity_bits(main_case, main_forwards):
    """2. The record's o' is f32(o * coef_f32) bit for bit on every visible Gaussian (F1 is built
    contraction-off with correctly rounded divide and sqrt); at the clamp, f32(o * sqrtf(0.000025f))."""
    cam, s, inputs, dC = main_case
    off, on = main_forwards
    vis = _np(on.radii) > 0
    o = s.opacities.reshape(-1)
    c32, c64, r64 = coef_f32(cam, inputs)
    want = compensated(o, c32)
    got = _records_opacity(on)
    assert vis.sum() > 4500
    np.testing.assert_array_equal(got[vis].view(np.uint32), want[vis].view(np.uint32))
    np.testing.assert_array_equal(_records_opacity(off)[vis].view(np.uint32), o[vis].view(np.uint32))
    clamped = vis & (r64 < 0.5 * R_CLAMP)
    assert clamped.sum() >= 100
    floor = (o * np.sqrt(np.float32(R_CLAMP))).astype(np.float32)
    np.testing.assert_array_equal(got[clamped].view(np.uint32), floor[clamped].view(np.uint32))


def _precomp_case():
    """2000 Gaussians / 200x120 with cov3D_precomp, colors_precomp, scale_modifier 1.7 (which a
    precomputed covariance ignores, in F1 and in the compensation alike) and a coloured background:
    F1 without SH rows, B2's cov3D branch."""
    import gsr_oracle
    cam = pkg("graphics").synthetic_camera(200, 120)
    s = aa_scene(cam, 2000, seed=SEED_PRECOMP)
    cov = np.stack([gsr_oracle.covariance(s.scales[i], 1.0, s.rotations[i]) for i in range(s.P)])
    colors = np.random.default_rng(5).uniform(0.0, 1.0, (s.P, 3)).astype(np.float32)
    inputs = dict(means3D=s.means3D, opacities=s.opacities, cov3D_precomp=cov, colors_precomp=colors)
    return cam, inputs, pkg("scene").make_dL_dpix(cam, seed=4), dict(scale_modifier=1.7, bg=(0.2, 0.5, 0.9))


@pytest.mark.parametrize("case", ["sh3", "precomp"])
def test_parity(case, main_case, rast, oracle):
    """3. Colour and every gradient tensor against the oracle run on the GPU's own o' plus
    apply_aa_chain.
    The scene seeds are chosen on the reference alone, by test_gpu_aux.test_parity_large_image's
    criterion: a (pixel, Gaussian) pair whose alpha lies within f32 rounding of the 1/255 cut can fall
    on either side of it under the GPU's exp2 and the oracle's expf.  Evaluated in f64 from the
    oracle's own preprocess run on o' = f32(o coef_f32), over every pair inside a Gaussian's tile
    rect.  5000 / 300x200: seed 4 keeps its closest pair farthest from the cut, |255 alpha - 1| >= 8.3e-6
    (seeds 0..5: 8.0e-7, 1.9e-6, 3.9e-6, 1.7e-6, 8.3e-6, 2.1e-6).  2000 / 200x120: seed 0, >= 2.2e-5
    (seeds 0..5: 2.2e-5, 1.5e-5, 2.1e-5, 1.8e-5, 2.8e-6, 9.2e-6).  The trainer test's scene (3000 /
    160x120, seed 3 as in test_gpu_depth_loss.py) has 5.7e-6."""
    if case == "sh3":
        cam, s, inputs, dC = main_case
        D, kw = 3, {}
    else:
        cam, inputs, dC, kw = _precomp_case()
        D = 0
    st = rast.forward(cam, **inputs, sh_degree=D, antialiasing=True, **kw)
    o_gpu, vis = _gpu_o_prime(st, inputs)
    # the GPU's o' is the reference's own (test 2 holds it bit for bit on the SH3 scene)
    want_o = compensated(inputs["opacities"], coef_f32(cam, inputs, kw.get("scale_modifier", 1.0))[0])
    np.testing.assert_array_equal(o_gpu[vis].view(np.uint32), want_o[vis].view(np.uint32))
    f, want, _ = aa_oracle(oracle, cam, inputs, D, dC, o_prime=o_gpu, **kw)
    _check_colour(st, f)
    g = rast.backward(st, dC)
    _check_grads(g, want)
    # the chain term is no rounding detail: without it the covariance leaf misses the bar by far
    _, nochain, _ = aa_oracle(oracle, cam, inputs, D, dC, o_prime=o_gpu, chain=False, **kw)
    k = "scales" if case == "sh3" else "cov3D"
    assert rel_l2(_np(g[k]).reshape(nochain[k].shape), nochain[k]) > 100 * GRAD_REL
    # B2 alone, from the gather's 2D gradients, carries the same flag
    g2 = rast.backward_preprocess(st, rast.backward_blend(st, dC))
    for key in g:
        assert torch.equal(g[key], g2[key]), key


@pytest.mark.parametrize("s2,antialiasing", CLOSED_FORM)
def test_closed_form_energy(s2, antialiasing, rast):
    """4. One isotropic sub-pixel Gaussian: the blended energy is 2 pi sqrt(det1) (o_eff - 1/255) within
    one pixel ring at the 1/255 cut -- with the flag, the energy of its true footprint."""
    cam, inputs, want, tol = closed_form_case(s2, antialiasing)
    st = rast.forward(cam, **inputs, sh_degree=0, antialiasing=antialiasing)
    got = float(st.color[0].double().sum())
    print(s2, antialiasing, got, want, tol)
    assert float(st.color[1:].abs().max()) == 0.0
    assert abs(got - want) <= tol


@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "invdepth"])
def test_aux_with_antialias(inverse, main_case, main_forwards, rast, oracle):
    """5. forward_aux(antialiasing=True): the colour is forward(antialiasing=True)'s bit for bit; depth,
    alpha and all gradients match aux_reference run on o', passed through apply_aa_chain."""
    cam, s, inputs, dC = main_case
    dD, dA = make_aux_grads(cam, seed=3)
    st = rast.forward_aux(cam, **inputs, sh_degree=3, inverse_depth=inverse, antialiasing=True)
    assert torch.equal(st.color, main_forwards[1].color) and torch.equal(st.radii, main_forwards[1].radii)
    o_gpu, vis = _gpu_o_prime(st, inputs)
    ref = aux_reference(oracle, cam, dict(inputs, opacities=o_gpu), 3, dC, dD, dA, inverse=inverse)
    for name, got, want in (("depth", st.depth, ref["depth"]), ("alpha", st.alpha, ref["alpha"])):
        a = _np(got)
        r = rel_l2(a, want)
        frac, worst = elementwise_misses(a, want, *ELEM_RGB)
        print(f"{name}: rel_l2 {r:.3e} misses {frac:.3e} worst {worst:.3e}")
        assert r <= IMG_REL and frac <= RGB_FLIPS, (name, r, frac)
    grads = {k: v for k, v in ref["grads"].items() if k != "dz_term"}
    want = apply_aa_chain(cam, inputs, grads)
    _check_grads(rast.backward_aux(st, dC, dD, dA), want)


def test_views_and_batch_with_antialias(rast):
    """6. Two cameras of test_gpu_views.py's shape: forward_views / backward_views with the flag are
    bit-identical to the per-view flagged calls (compared as test_views_equal_single_views compares),
    and forward_batch with the flag to single forwards."""
    cams = _cams(320, 250, 2)
    s = aa_scene(pkg("graphics").synthetic_camera(320, 240), 5000, seed=21)
    args = (s.means3D, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest)
    kw = dict(sh_degree=3, bg=(0.1, 0.2, 0.3), antialiasing=True)
    st = rast.forward_views(cams, *args, **kw)
    V, H, W = 2, 250, 320
    gen = torch.Generator("cuda").manual_seed(5)
    dpix = torch.rand((V, 3, H, W), device="cuda", generator=gen)
    gv = rast.backward_views(st, dpix)
    batch = rast.forward_batch(cams, *args, **kw)
    leaf = None
    for v, cam in enumerate(cams):
        a = rast.forward(cam, *args, **kw)
        assert torch.equal(a.color, st.color[v]) and torch.equal(a.radii, st.radii[v]), v
        assert torch.equal(a.color, batch[v].color) and torch.equal(a.radii, batch[v].radii), v
        assert not torch.equal(a.color, rast.forward(cam, *args, sh_degree=3, bg=(0.1, 0.2, 0.3)).color)
        ga = rast.backward(a, dpix[v])
        gb = rast.backward(batch[v], dpix[v])  # the batch's states carry the flag too
        for k in ga:
            assert torch.equal(ga[k], gb[k]), (k, v)
        for k in ("means2D", "conic"):
            assert torch.equal(ga[k], gv[k][v]), (k, v)
        leaf = {k: t.clone() for k, t in ga.items() if k not in ("means2D", "conic")} if leaf is None else \
            {k: leaf[k] + ga[k] for k in leaf}
    for k in leaf:
        assert torch.equal(leaf[k], gv[k]), k


def test_autograd_and_render_match_cabi(main_case, main_forwards, rast):
    """7. rasterize_gaussians(antialiasing=True) and render(pipe.antialiasing=True) are the C-ABI flagged
    forward and backward bit for bit; a flagged forward's state handed to a backward with the flag
    stripped is refused (GSR_ERR_LAYOUT)."""
    native, R, M = pkg("native"), pkg("rasterizer"), pkg("model")
    cam, s, inputs, dC = main_case
    off, on = main_forwards
    t = lambda a: torch.tensor(a, device="cuda", requires_grad=True)
    leaves = {k: t(v) for k, v in inputs.items()}
    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii = R.rasterize_gaussians(cam, leaves["means3D"], m2d, leaves["opacities"], sh_dc=leaves["sh_dc"],
                                         sh_rest=leaves["sh_rest"], scales=leaves["scales"],
                                         rotations=leaves["rotations"], sh_degree=3, antialiasing=True)
    assert torch.equal(on.color, color.detach()) and torch.equal(on.radii, radii)
    names = list(leaves)
    dCt = torch.tensor(dC, device="cuda")
    grads = torch.autograd.grad((color * dCt).sum(), [leaves[k] for k in names] + [m2d])
    g = rast.backward(on, dC)
    for k, got in zip(names + ["means2D"], grads):
        assert torch.equal(got.reshape(g[k].shape), g[k]), k
    # the aux Function carries the flag as well
    ca, da, aa, ra = R.rasterize_gaussians_aux(cam, leaves["means3D"], m2d, leaves["opacities"],
                                               sh_dc=leaves["sh_dc"], sh_rest=leaves["sh_rest"],
                                               scales=leaves["scales"], rotations=leaves["rotations"], sh_degree=3,
                                               antialiasing=True)
    assert torch.equal(ca.detach(), on.color)
    ga = torch.autograd.grad((ca * dCt).sum(), [leaves["scales"]])[0]
    assert torch.equal(ga, g["scales"])
    # render(): the model's activations feed both sides
    model = M.GaussianModel.from_scene(s, "cuda")
    bg = torch.zeros(3, device="cuda")
    out = R.render(cam, model, R.PipelineParams(antialiasing=True), bg)
    act = dict(means3D=model.get_xyz.detach(), opacities=model.get_opacity.detach(),
               scales=model.get_scaling.detach(), rotations=model.get_rotation.detach(),
               sh_dc=model.features_dc.detach(), sh_rest=model.features_rest.detach())
    ref = rast.forward(cam, **act, sh_degree=3, antialiasing=True)
    assert torch.equal(out["render"], ref.color) and torch.equal(out["radii"], ref.radii)
    assert not torch.equal(out["render"], R.render(cam, model, R.PipelineParams(), bg)["render"])
    (out["render"] * dCt).sum().backward()
    gr = rast.backward(ref, dC)
    assert torch.equal(model.get_xyz.grad, gr["means3D"])
    assert torch.equal(out["viewspace_points"].grad, gr["means2D"])
    # the flag stripped from a flagged forward's state, and set on an unflagged one's
    for st, flags in ((on, on.settings.flags & ~native.GSR_FLAG_ANTIALIAS),
                      (off, off.settings.flags | native.GSR_FLAG_ANTIALIAS)):
        keep = st.settings.flags
        st.settings.flags = flags
        try:
            with pytest.raises(RuntimeError, match=rf"\({native.GSR_ERR_LAYOUT}\).*GSR_FLAG_ANTIALIAS"):
                rast.backward(st, dC)
        finally:
            st.settings.flags = keep


def test_trainer_with_antialias(oracle):
    """8. GaussianTrainer.step: antialiasing=False is the default step bit for bit; with True, exp_avg
    after one step is 0.1 x the gradients of the CPU composite (test_gpu_depth_loss.py's, with
    apply_aa_chain inserted) within that test's 1e-4 rel-L2; a depth-supervised flagged step runs
    under its bound with the device-side guard clean."""
    Tr = pkg("trainer")
    cam = pkg("graphics").synthetic_camera(160, 120)
    s = aa_scene(cam, 3000, seed=3)
    gt = np.random.default_rng(4).random((3, 120, 160)).astype(np.float32)
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")

    def trainer(**opt):
        tr = Tr.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                                s.raw_rotations, max_sh_degree=3, opt=Tr.OptimizationParams(**opt), device="cuda")
        tr.active_sh_degree = 3
        return tr

    a, b, c = trainer(), trainer(antialiasing=False), trainer(antialiasing=True)
    oa, ob, oc = (t.step(1, cam, tt(gt), densify=False) for t in (a, b, c))
    for k in Tr.GROUPS:
        assert torch.equal(a.params[k], b.params[k]) and torch.equal(a.exp_avg[k], b.exp_avg[k]), k
    assert torch.equal(oa["image"], ob["image"]) and not torch.equal(oa["image"], oc["image"])
    # CPU composite on the GPU's own o'
    sc_, q_, o_ = T.activate(s.raw_scales, s.raw_rotations, s.raw_opacities.reshape(-1, 1))
    inputs = dict(means3D=s.means3D, opacities=o_.reshape(-1), scales=sc_, rotations=q_, sh_dc=s.sh_dc,
                  sh_rest=s.sh_rest)
    o_gpu, vis = _gpu_o_prime(oc["state"], inputs)
    f = oracle.forward(cam, s.means3D, o_gpu, scales=sc_, rotations=q_, sh_dc=s.sh_dc, sh_rest=s.sh_rest,
                       sh_degree=3)
    loss, _, _, dimg = T.ssim_loss(f.color.astype(np.float32), gt, 0.2)
    st = oc["stats"].cpu().numpy()
    assert abs(st[0] - loss) <= 1e-4 * abs(loss)
    g = apply_aa_chain(cam, inputs, f.state.backward(dimg))
    ds, dq, do = T.raw_grads(s.raw_scales, s.raw_rotations, s.raw_opacities.reshape(-1, 1), g["scales"],
                             g["rotations"], g["opacities"].reshape(-1, 1))
    graw = {"xyz": g["means3D"], "f_dc": g["sh_dc"], "f_rest": g["sh_rest"], "opacity": do, "scaling": ds,
            "rotation": dq}
    for k in Tr.GROUPS:
        m = c.exp_avg[k].cpu().numpy()
        r = rel_l2(m, 0.1 * np.asarray(graw[k], np.float64).reshape(m.shape))
        print(k, "exp_avg rel_l2", r)
        assert r <= 1e-4, (k, r)
    # depth-supervised, flagged: the second step renders under the bound, guarded on the device
    d = trainer(antialiasing=True)
    target = tt(np.full((120, 160), 0.2, np.float32))
    for it in (1, 2):
        od = d.step(it, cam, tt(gt), densify=False, gt_depth=target)
        assert "depth_stats" in od
        assert od["state"].settings.flags & pkg("native").GSR_FLAG_ANTIALIAS
        assert od["state"].buffers.layout & pkg("native").GSR_LAYOUT_AUX
    torch.cuda.synchronize()
    d.binning.poll()
    assert d.binning.exact_reads == 1 and d.binning.overflows == 0
    assert all(bool(torch.isfinite(d.params[k]).all()) for k in Tr.GROUPS)


def test_degenerate_inputs(rast):
    """9. 64 Gaussians that are edge-on discs (one scale 1e-5) and 1e-6-scale points: finite colour and
    gradients, o' >= 0.005 o, and no gradient through coef where the clamp holds -- there the flagged
    `scales` gradient is the chain-free one (the unflagged B2's on the same 2D gradients)."""
    native = pkg("native")
    cam = pkg("graphics").synthetic_camera(64, 48)
    s = pkg("scene").make_scene(cam, 64, max_sh_degree=1, seed=9)
    s.scales[:32, 2] = 1e-5
    s.rotations[:32] = np.array([0.70710678, 0.70710678, 0.0, 0.0], np.float32)  # the thin axis across the view
    s.scales[32:] = 1e-6
    s.opacities[32:] = 0.98  # o' = 0.0049: still above 1/255 within a third of a pixel of the centre
    inputs = dict(means3D=s.means3D, opacities=s.opacities, scales=s.scales, rotations=s.rotations, sh_dc=s.sh_dc,
                  sh_rest=s.sh_rest)
    dC = pkg("scene").make_dL_dpix(cam, seed=10)
    st = rast.forward(cam, **inputs, sh_degree=1, antialiasing=True)
    g = rast.backward(st, dC)
    assert bool(torch.isfinite(st.color).all())
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    vis = _np(st.radii) > 0
    assert vis[32:].sum() > 20
    o = s.opacities.reshape(-1)
    got = _records_opacity(st)
    assert (got[vis] >= (o[vis] * np.float32(0.005)) * np.float32(1 - 1e-6)).all() and (got[vis] <= o[vis]).all()
    # the chain-free gradient: the plain B2 on the flagged pass's own 2D gradients (its opacity slot is
    # dL/do', which the covariance gradients never read)
    grad2d = rast.backward_blend(st, dC)
    st.settings.flags &= ~native.GSR_FLAG_ANTIALIAS
    st.buffers.layout &= ~native.GSR_LAYOUT_ANTIALIAS
    free = rast.backward_preprocess(st, grad2d)
    _, _, r64 = coef_f32(cam, inputs)
    clamped = vis & (r64 < 0.5 * R_CLAMP)
    assert clamped[32:].sum() > 20
    assert torch.equal(g["scales"][torch.tensor(clamped)], free["scales"][torch.tensor(clamped)])
    assert float(g["scales"][torch.tensor(clamped)].abs().sum()) > 0
