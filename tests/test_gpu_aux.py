"""GPU parity of the depth and alpha outputs (gsr_forward_aux / gsr_backward_aux, the autograd
Function over them and render(return_depth=True)) against the CPU oracle composed as in
tests/test_native_aux.py (`aux_reference`, pinned there against fp64 autograd).

Bars (the parity suite's, by value): images rel-L2 <= 1e-4 and ELEM_RGB = (1e-4, 1e-3) with at most
RGB_FLIPS = 1e-5 of the values outside it, the worst depth miss <= max(v) / 100 (one alpha >= 1/255
flip moves a pixel by at most ~v / 255); gradients rel-L2 <= 1e-4 and ELEM_GRAD = (1e-3, 1e-2) with
at most GRAD_FLIPS = 1e-3 outside it (the banded-sheet scene: 2e-3, as in
test_chunk_checkpoints_with_finished_stripes).  Each scene is the smallest that reaches its path.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_fixture, pkg, rel_l2
from test_native_aux import aux_reference, make_aux_grads
from test_gpu_parity import _banded_front_scene, elementwise_misses

pytestmark = pytest.mark.gpu

IMG_REL, GRAD_REL = 1e-4, 1e-4
ELEM_RGB, ELEM_GRAD = (1e-4, 1e-3), (1e-3, 1e-2)
RGB_FLIPS, GRAD_FLIPS = 1e-5, 1e-3
GRAD_KEYS = ["means2D", "conic", "opacities", "means3D", "sh_dc", "sh_rest", "scales", "rotations", "colors",
             "cov3D"]


@pytest.fixture(scope="module")
def rast():
    return pkg("rasterizer").CAbiRasterizer("cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _scene_inputs(s):
    return dict(means3D=s.means3D, opacities=s.opacities, scales=s.scales, rotations=s.rotations, sh_dc=s.sh_dc,
                sh_rest=s.sh_rest)


def _check_images(st, ref, inverse):
    """Colour, discrete outputs, depth and alpha of a forward_aux against the reference."""
    np.testing.assert_array_equal(_np(st.radii), ref["radii"])
    assert st.num_rendered == ref["num_rendered"]
    cfrac, cworst = elementwise_misses(_np(st.color), ref["color"], *ELEM_RGB)
    print(f"colour: rel_l2 {rel_l2(_np(st.color), ref['color']):.3e} misses {cfrac:.3e} worst {cworst:.3e}")
    assert rel_l2(_np(st.color), ref["color"]) <= IMG_REL
    assert cfrac <= RGB_FLIPS and cworst <= 0.01, (cfrac, cworst)
    vis = ref["radii"] > 0
    vmax = 0.0
    if vis.any():
        z = ref["z"][vis].astype(np.float64)
        vmax = float((1.0 / z).max() if inverse else z.max())
    for name, got, want, cap in (("depth", st.depth, ref["depth"], vmax / 100.0), ("alpha", st.alpha, ref["alpha"], 0.01)):
        a = _np(got)
        r = rel_l2(a, want)
        frac, worst = elementwise_misses(a, want, *ELEM_RGB)
        print(f"{name}: rel_l2 {r:.3e} misses {frac:.3e} worst {worst:.3e} (cap {cap:.3e})")
        if frac > 0:  # where: a threshold flip shows in colour, depth and alpha at the same pixel
            i = int(np.abs(a - want).argmax())
            y, x = divmod(i, a.shape[1])
            print(f"  worst {name} pixel ({x}, {y}): got {a[y, x]:.6f} want {want[y, x]:.6f}; colour diff there "
                  f"{np.abs(_np(st.color)[:, y, x] - ref['color'][:, y, x]).max():.3e}")
        assert r <= IMG_REL, (name, r)
        assert frac <= RGB_FLIPS and worst <= cap, (name, frac, worst, cap)


def _check_grads(g_gpu, ref, flips=GRAD_FLIPS):
    worst = {}
    for k in GRAD_KEYS:
        if k in g_gpu:
            want = ref["grads"][k]
            a = _np(g_gpu[k]).reshape(want.shape)
            r = rel_l2(a, want)
            worst[k] = elementwise_misses(a, want, *ELEM_GRAD)
            d = np.abs(a.astype(np.float64) - want).reshape(a.shape[0], -1).max(1) if a.size else np.zeros(0)
            top = np.sort(d)[::-1][:3] if d.size else []
            print(f"grad {k}: rel_l2 {r:.3e} misses {worst[k][0]:.3e} |ref| {np.linalg.norm(want):.3e} "
                  f"largest per-Gaussian errors {[float(f'{v:.3e}') for v in top]}")
            assert r <= GRAD_REL, (k, r)
    assert max(v[0] for v in worst.values()) <= flips, worst


def _run(rast, oracle, cam, inputs, D, dC, dD, dA, inverse, bg=(0.0, 0.0, 0.0), flips=GRAD_FLIPS):
    st = rast.forward_aux(cam, **inputs, sh_degree=D, bg=bg, inverse_depth=inverse)
    ref = aux_reference(oracle, cam, inputs, D, dC, dD, dA, inverse=inverse, bg=bg)
    _check_images(st, ref, inverse)
    g = rast.backward_aux(st, dC, dD, dA)
    _check_grads(g, ref, flips)
    return st, g, ref


# ---- case 1: small-image path (247 tiles < 4096: four-wave F6, prefetching B1; partial edge tiles) ----
@pytest.fixture(scope="module")
def case1():
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(300, 200)
    s = sc.make_scene(cam, 5000, max_sh_degree=3, seed=1)
    dC = sc.make_dL_dpix(cam, seed=2)
    dD, dA = make_aux_grads(cam, seed=3)
    return cam, s, _scene_inputs(s), dC, dD, dA


@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "invdepth"])
def test_parity_small_image(inverse, case1, rast, oracle):
    cam, s, inputs, dC, dD, dA = case1
    _run(rast, oracle, cam, inputs, 3, dC, dD, dA, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "invdepth"])
def test_depth_only_loss(inverse, case1, rast, oracle):
    """dL/dcolor = dL/dalpha = 0 (the latter as NULL): every gradient comes from the depth image,
    and the dL/dz -> dL/dmeans3D term stands two orders above the rel-L2 bar, so leaving it out
    (or mis-scaling it under inverse depth) fails the means3D check."""
    cam, s, inputs, dC, dD, dA = case1
    zero = np.zeros_like(dC)
    st, g, ref = _run(rast, oracle, cam, inputs, 3, zero, dD, None, inverse)
    gm, dz = ref["grads"]["means3D"], ref["grads"]["dz_term"]
    assert np.linalg.norm(dz) > 100 * GRAD_REL * np.linalg.norm(gm)
    assert float(g["sh_dc"].abs().max()) == 0.0 and float(g["sh_rest"].abs().max()) == 0.0


# ---- case 2: large-image path (4096 tiles: two-wave F6 at 7 waves per SIMD, plain-loop B1) ----
@pytest.fixture(scope="module")
def case2():
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(1024, 1024)
    assert cam.grid[0] * cam.grid[1] == 4096
    s = sc.make_scene(cam, 20000, max_sh_degree=3, seed=5)
    dC = sc.make_dL_dpix(cam, seed=6)
    dD, dA = make_aux_grads(cam, seed=7)
    return cam, _scene_inputs(s), dC, dD, dA


def test_parity_large_image(case2, rast, oracle):
    """The aux launches choose their instantiations by tile count as the plain ones do, so the
    large-image pair gets its own case: 20000 Gaussians at 1024x1024 (4096 tiles), SH1.
    The scene seed is chosen on the reference alone.  A (pixel, Gaussian) pair whose alpha lies within
    f32 rounding of the 1/255 cut can fall on either side of it under the GPU's exp2 and the oracle's
    expf (one such flip moves a faint Gaussian's whole gradient, and at 20000 Gaussians that alone is
    ~1e-4 of a tensor's norm).  Of make_scene's seeds 4..9, evaluated in f64 from the oracle's own
    preprocess, seed 5 keeps its closest pair farthest from the cut (|255 alpha - 1| >= 7.0e-7; the
    others come within 1.4e-7, 7.7e-8, 4.5e-7, 2.8e-7 and 1.5e-7).  Seed 4 was measured on the MI355X:
    its 1.4e-7 pair (pixel (753, 536), Gaussian 15674) flipped, in the colour pass as well, and put the
    opacity gradient at rel-L2 1.39e-4 (0.29 of the tensor's 2063 from that one Gaussian)."""
    cam, inputs, dC, dD, dA = case2
    _run(rast, oracle, cam, inputs, 1, dC, dD, dA, False)


def _chunk_tables(st, cam):
    native = pkg("native")
    tiles, S = cam.grid[0] * cam.grid[1], native.TERM_STRIDE
    term = _np(st.view(native.VIEW_TERM, torch.int32, tiles * S)).view(np.uint32).reshape(tiles, S)
    pool = int(native.load_hip().gsr_ck_pool_slots(st.buffers.capacity, cam.width, cam.height))
    live = _np(st.view(native.VIEW_CK_LIVE, torch.uint8, pool * 4)).reshape(pool, 4)
    rng = _np(st.view(native.VIEW_RANGES, torch.int32, 2 * tiles)).view(np.uint32).reshape(tiles, 2)
    return term, live, rng, pool


# ---- case 3: chunk checkpoints, some starting with finished stripes ----
def test_chunk_checkpoints_carry_depth(rast, oracle):
    gr, sc = pkg("graphics"), pkg("scene")
    native = pkg("native")
    cam = gr.synthetic_camera(256, 192)
    s = _banded_front_scene(cam, 20000, seed=21)
    dC = sc.make_dL_dpix(cam, seed=22)
    dD, dA = make_aux_grads(cam, seed=23)
    # the banded sheets put many pairs near the T >= 1e-4 cut: 2e-3 element misses, as in
    # test_chunk_checkpoints_with_finished_stripes (rel-L2 stays at 1e-4)
    st, g, ref = _run(rast, oracle, cam, _scene_inputs(s), 1, dC, dD, dA, False, flips=2e-3)
    term, live, rng, pool = _chunk_tables(st, cam)
    tiles, S = term.shape
    opened = term[:, 1:] != 0xFFFFFFFF
    assert opened.sum() > tiles  # chunks >= 1 opened, more than one per tile on average
    fixed = pool == tiles * (S - 1)
    ids = np.array([native.ck_slot(fixed, int(rng[t, 0]), t, c + 1) for t, c in zip(*np.nonzero(opened))])
    on = live[ids]
    assert (on[:, :2] == 0).mean() > 0.25 and (on[:, 3] == 1).mean() > 0.5, on.mean(0)  # finished stripes at starts


# ---- case 4: deep lists, fixed slots, at least one chunk merge ----
def test_deep_lists_merge_keeps_depth(rast, oracle):
    gr, sc = pkg("graphics"), pkg("scene")
    native = pkg("native")
    P = 2000
    cam = gr.synthetic_camera(64, 64)
    s = sc.make_scene(cam, P, max_sh_degree=1, seed=71)
    rng = np.random.default_rng(71)
    z = np.linspace(4.0, 8.0, P)
    xy = rng.uniform(-0.4, 0.4, (P, 2)) * z[:, None] * np.array([cam.tanfovx, cam.tanfovy])
    s.means3D = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    s.scales = np.full((P, 3), 6.0, np.float32)
    s.opacities = np.full((P, 1), 0.005, np.float32)
    dC = sc.make_dL_dpix(cam, seed=72)
    dD, dA = make_aux_grads(cam, seed=73)
    st, g, ref = _run(rast, oracle, cam, _scene_inputs(s), 1, dC, dD, dA, False)
    term, live, rng_t, pool = _chunk_tables(st, cam)
    tiles, S = term.shape
    assert pool == tiles * (S - 1)  # the fixed 31-per-tile layout
    opened = term[:, 1:] != 0xFFFFFFFF
    assert opened.sum(1).max() >= 15
    # > 31 * 48 entries per tile need more than 31 chunks of the base quota: F6 merged at least once
    n = rng_t[:, 1] - rng_t[:, 0]
    assert int(n.max()) > 31 * native.CK_DIV


# ---- case 5: precomputed colour and covariance, coloured background ----
def test_precomputed_inputs(rast, oracle):
    path = [p for p in GOLDEN if os.path.basename(p) == "precomp_48x40.npz"][0]
    meta, cam, inp, out = load_fixture(path)
    inputs = dict(means3D=inp["means3D"], opacities=inp["opacities"], colors_precomp=inp["colors_precomp"],
                  cov3D_precomp=inp["cov3D_precomp"])
    bg = tuple(float(v) for v in inp["bg"])
    assert max(bg) > 0
    dD, dA = make_aux_grads(cam, seed=11)
    for inverse in (False, True):
        st, g, ref = _run(rast, oracle, cam, inputs, 0, inp["dL_dpix"], dD, dA, inverse, bg=bg)
        # no background in depth or alpha: a black background gives the same two images, bit for bit
        # (the reference's are rendered over black), while the colour does change
        black = rast.forward_aux(cam, **inputs, sh_degree=0, inverse_depth=inverse)
        assert torch.equal(black.depth, st.depth) and torch.equal(black.alpha, st.alpha)
        assert not torch.equal(black.color, st.color)


# ---- case 6: colour untouched ----
def _colour_path_unchanged(rast, cam, inputs, D, dC):
    """forward_aux against forward, and backward_aux without aux gradients and the plain backward of
    aux buffers against backward: bitwise equal (both sides are the library's own: no tolerance)."""
    native = pkg("native")
    a = rast.forward(cam, **inputs, sh_degree=D)
    for inverse in (False, True):
        b = rast.forward_aux(cam, **inputs, sh_degree=D, inverse_depth=inverse)
        assert torch.equal(a.color, b.color) and torch.equal(a.radii, b.radii)
        K = a.num_rendered
        assert b.num_rendered == K
        for what in (native.VIEW_SORTED_GID, native.VIEW_SORTED_TILE):
            assert torch.equal(a.view(what, torch.int32, K), b.view(what, torch.int32, K))
        ga, gb = rast.backward(a, dC), rast.backward_aux(b, dC, None, None)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        # the plain backward accepts aux buffers (colour gradients only)
        gc = rast.backward(b, dC)
        for k in ga:
            assert torch.equal(ga[k], gc[k]), k
    return a


def test_colour_path_unchanged(case1, rast):
    cam, s, inputs, dC, dD, dA = case1
    a = _colour_path_unchanged(rast, cam, inputs, 3, dC)
    with pytest.raises(RuntimeError, match="GSR_LAYOUT_AUX"):
        rast.backward_aux(a, dC, dD, dA)  # plain buffers hold no depth sums
    with pytest.raises(RuntimeError, match="full images only"):
        rast.forward_aux(cam, **inputs, sh_degree=3, tile_rows=(0, 4))


def test_colour_path_unchanged_large_image(case2, rast):
    """The other side of the blend launchers' tile-count selection, which the plain and the aux
    launch share: 4096 tiles is the smallest image on the two-wave F6 and the plain-loop B1."""
    cam, inputs, dC, dD, dA = case2
    _colour_path_unchanged(rast, cam, inputs, 1, dC)


# ---- case 7: edges ----
def test_empty_and_culled(rast):
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(64, 48)
    s = sc.make_scene(cam, 50, max_sh_degree=1)
    means = s.means3D.copy()
    means[:, 2] = -2.0
    st = rast.forward_aux(cam, means, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest, sh_degree=1,
                          bg=(0.1, 0.2, 0.3), debug=True)
    assert st.num_rendered == 0
    assert float(st.depth.abs().max()) == 0.0 and float(st.alpha.abs().max()) == 0.0
    one = np.ones((48, 64), np.float32)
    g = rast.backward_aux(st, np.ones((3, 48, 64), np.float32), one, one)
    assert all(float(v.abs().max()) == 0.0 for v in g.values())
    st0 = rast.forward_aux(cam, np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)), np.zeros((0, 4)),
                           np.zeros((0, 1, 3)), None, sh_degree=0, bg=(1, 1, 1))
    assert float(st0.color.min()) == 1.0
    assert float(st0.depth.abs().max()) == 0.0 and float(st0.alpha.abs().max()) == 0.0
    g0 = rast.backward_aux(st0, np.ones((3, 48, 64), np.float32), one, one)
    assert all(v.numel() == 0 for v in g0.values())


def test_capacity_bound_and_overflow(case1, rast):
    cam, s, inputs, dC, dD, dA = case1
    exact = rast.forward_aux(cam, **inputs, sh_degree=3)
    K = exact.num_rendered
    ge = rast.backward_aux(exact, dC, dD, dA)
    st = rast.forward_aux(cam, **inputs, sh_degree=3, max_rendered=K + 1000)
    assert st.buffers.num_rendered == -1 and st.buffers.capacity == K + 1000  # no host read
    assert st.num_rendered == K
    for a, b in ((st.color, exact.color), (st.depth, exact.depth), (st.alpha, exact.alpha)):
        assert torch.equal(a, b)
    g = rast.backward_aux(st, dC, dD, dA)
    for k in ge:
        assert torch.equal(g[k], ge[k]), k
    st = rast.forward_aux(cam, **inputs, sh_degree=3, max_rendered=K // 2)
    g = rast.backward_aux(st, dC, dD, dA)
    torch.cuda.synchronize()
    with pytest.raises(OverflowError):
        st.num_rendered
    assert all(bool(torch.isfinite(t).all()) for t in (st.color, st.depth, st.alpha, *g.values()))


# ---- case 8: autograd ----
@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "invdepth"])
def test_autograd_matches_cabi(inverse, case1, rast):
    cam, s, inputs, dC, dD, dA = case1
    R = pkg("rasterizer")
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)
    leaves = {k: t(v) for k, v in inputs.items()}
    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, depth, alpha, radii = R.rasterize_gaussians_aux(
        cam, leaves["means3D"], m2d, leaves["opacities"], sh_dc=leaves["sh_dc"], sh_rest=leaves["sh_rest"],
        scales=leaves["scales"], rotations=leaves["rotations"], sh_degree=3, inverse_depth=inverse)
    st = rast.forward_aux(cam, **inputs, sh_degree=3, inverse_depth=inverse)
    assert torch.equal(st.color, color.detach()) and torch.equal(st.radii, radii)
    assert torch.equal(st.depth, depth.detach()) and torch.equal(st.alpha, alpha.detach())
    tt = lambda a: torch.tensor(a, device=dev)
    loss = (color * tt(dC)).sum() + (depth * tt(dD)).sum() + (alpha * tt(dA)).sum()
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names] + [m2d])
    g = rast.backward_aux(st, dC, dD, dA)
    for k, got in zip(names + ["means2D"], grads):
        assert torch.equal(got.reshape(g[k].shape), g[k]), k


def test_render_returns_depth_when_asked(rast):
    gr, sc = pkg("graphics"), pkg("scene")
    R, M = pkg("rasterizer"), pkg("model")
    cam = gr.synthetic_camera(192, 144)
    s = sc.make_scene(cam, 3000, max_sh_degree=3, seed=3)
    model = M.GaussianModel.from_scene(s, "cuda")
    bg = torch.zeros(3, device="cuda")
    base = R.render(cam, model, R.PipelineParams(), bg)
    assert set(base) == {"render", "viewspace_points", "visibility_filter", "radii"}  # exactly today's keys
    out = R.render(cam, model, R.PipelineParams(), bg, return_depth=True)
    assert set(out) == set(base) | {"depth", "alpha"}
    assert torch.equal(out["render"], base["render"]) and torch.equal(out["radii"], base["radii"])
    assert out["depth"].shape == out["alpha"].shape == (cam.height, cam.width)
    inv = R.render(cam, model, R.PipelineParams(), bg, return_depth=True, inverse_depth=True)
    assert torch.equal(inv["alpha"], out["alpha"]) and not torch.equal(inv["depth"], out["depth"])
    # a depth loss alone reaches the geometry leaves and the screen-space gradient
    (out["depth"] / out["alpha"].clamp_min(1e-3)).mean().backward()
    assert float(out["viewspace_points"].grad.abs().sum()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert float(model.get_xyz.grad.abs().sum()) > 0


# ---- case 9: determinism ----
def test_deterministic(case1, rast):
    cam, s, inputs, dC, dD, dA = case1
    a = rast.forward_aux(cam, **inputs, sh_degree=3)
    b = rast.forward_aux(cam, **inputs, sh_degree=3)
    for x, y in ((a.color, b.color), (a.depth, b.depth), (a.alpha, b.alpha)):
        assert torch.equal(x, y)
    ga, gb = rast.backward_aux(a, dC, dD, dA), rast.backward_aux(b, dC, dD, dA)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
