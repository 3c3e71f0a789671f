"""The HIP kernels on the edge scene (tests/test_edge_reference.py): a posed, rolled camera over
Gaussians outside the guard band in x and in y, behind the camera, on both sides of the near plane,
with saturated alpha, terminated pixels, clamped SH channels and precomputed inputs.

(a) against the CPU oracle at the parity suite's bars (test_gpu_parity._compare as it stands: radii,
    num_rendered, the sorted (tile, gid) list and the ranges bit-exact, image and gradients), plus the
    depth keys and tiles_touched bit-exact -- F1's keys under a rotated view;
(b) against float64 autograd with the kernels' conventions (band_grad and alpha_clamp_grad "upstream"):
    every gradient tensor rel-L2 <= GRAD_REL over all visible rows AND over each class's rows, at most
    GRAD_FLIPS of the values outside ELEM_GRAD, rows of culled Gaussians exactly zero, image <= RGB_REL;
    colour, aux depth, and aux inverse depth with anti-aliasing (depth and alpha at test_gpu_aux's bars);
(c) the same bits by every route: the split backward, recomputed SH clamp bits, two bands, the libtorch
    Function, a view of a batch.

The f32 oracle's own distance to float64 on these cases is <= 3.0e-5 (any tensor, any class; the
near-plane rows carry it), so GRAD_REL = 1e-4 leaves 3x over an f32 implementation's measured floor.
The GPU's measured worst per tensor and class is printed by (b) and recorded in DESIGN 9i.
"""
import math

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2
from test_edge_reference import BG, CASES, SIZES, compare_grads, edge_case, fp64_reference, loss_weights, oracle_kwargs
from test_gpu_aux import ELEM_RGB as AUX_ELEM, IMG_REL as AUX_REL, RGB_FLIPS as AUX_FLIPS
from test_gpu_parity import GRAD_FLIPS, GRAD_REL, RGB_REL, _compare, elementwise_misses

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rast():
    return pkg("rasterizer").CAbiRasterizer("cuda")


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- (a) against the oracle
@pytest.mark.parametrize("size,config", CASES)
def test_edge_scene_against_oracle(size, config, rast, oracle):
    native = pkg("native")
    case = edge_case(size, config)
    cam, kw = case["cam"], oracle_kwargs(case["inputs"])
    P = len(case["visible"])
    st = rast.forward(cam, bg=BG, **kw)
    f = oracle.forward(cam, bg=BG, **kw)
    np.testing.assert_array_equal(f.radii > 0, case["visible"])
    dk = _np(st.view(native.VIEW_DEPTH_KEY, torch.int32, P)).view(np.uint32)
    pre = f.state.preprocess()
    vis = f.radii > 0
    np.testing.assert_array_equal(dk[vis], pre["depth"][vis].view(np.uint32))
    assert np.all(dk[~vis] == 0xFFFFFFFF)
    tt = _np(st.view(native.VIEW_TILES_TOUCHED, torch.int32, P)).view(np.uint32)
    np.testing.assert_array_equal(tt, pre["tiles_touched"])
    worst = _compare(st, f, loss_weights(size)[0], rast)
    print(f"\n{size} {config} vs oracle: K {st.num_rendered}, ELEM_GRAD misses {({k: v[0] for k, v in worst.items()})}")


# ---------------------------------------------------------------- (b) against float64
FP64_CASES = [(s, "sh3", m) for s in SIZES for m in ("colour", "aux", "aux_inverse_antialias")] + [
    ("P600_96x64", "precomp", "colour"), ("P600_96x64", "precomp", "aux"), ("P600_96x64", "precomp", "aux_inverse_antialias"),
    ("P600_100x70", "precomp", "aux_inverse_antialias"), ("P257_48x40", "precomp", "colour"),
    ("P600_100x70", "sh0", "colour"), ("P257_48x40", "sh0", "aux")]


def _gpu_run(rast, case, mode):
    cam, kw = case["cam"], oracle_kwargs(case["inputs"])
    dC, dD, dA = loss_weights(case["size"])
    if mode == "colour":
        st = rast.forward(cam, bg=BG, **kw)
        return st, rast.backward(st, dC)
    inv = mode == "aux_inverse_antialias"
    st = rast.forward_aux(cam, bg=BG, antialiasing=inv, inverse_depth=inv, **kw)
    return st, rast.backward_aux(st, dC, dD, dA)


@pytest.mark.parametrize("size,config,mode", FP64_CASES)
def test_edge_scene_against_float64(size, config, mode, rast):
    case = edge_case(size, config)
    vis = case["visible"]
    ref = fp64_reference(size, config, mode)
    st, g = _gpu_run(rast, case, mode)
    np.testing.assert_array_equal(_np(st.radii), case["geom"]["radius"].numpy())
    r = rel_l2(_np(st.color), ref["color"])
    print(f"\n{size} {config} {mode}: image rel-L2 {r:.2e}")
    assert r <= RGB_REL
    if mode != "colour":
        vmax = float(np.abs(ref["pre"]["value"].detach().numpy()[vis]).max())
        for name, got, cap in (("depth", st.depth, vmax / 100.0), ("alpha", st.alpha, 0.01)):
            a, want = _np(got), ref[name]
            rr = rel_l2(a, want)
            frac, worst = elementwise_misses(a, want, *AUX_ELEM)
            print(f"{name}: rel-L2 {rr:.2e}, outside ELEM_RGB {frac:.2e} (worst {worst:.2e}, cap {cap:.2e})")
            assert rr <= AUX_REL, (name, rr)
            assert frac <= AUX_FLIPS and worst <= cap, (name, frac, worst, cap)
    got = {k: _np(v) for k, v in g.items()}
    rel, miss = compare_grads(got, ref["grads"], case, f"GPU vs fp64 (upstream conventions), {size} {config} {mode}")
    assert set(k for k, _ in rel) >= ({"means2D", "means3D", "opacities"} | ({"colors", "cov3D"} if config == "precomp" else
                                                                             {"scales", "rotations", "sh_dc"}))
    assert max(rel.values()) <= GRAD_REL, max(rel.items(), key=lambda kv: kv[1])
    assert max(miss.values()) <= GRAD_FLIPS, miss
    for k, v in got.items():
        assert not v.reshape(len(vis), -1)[~vis].any(), k  # culled: exactly zero, both culls


def test_plain_autograd_reference_fails_the_same_kernels(rast):
    """What (b) is worth: against the plain-autograd forms of the two switches the same GPU gradients
    miss the bar by two orders of magnitude, on the out-of-band and opaque classes and on no other."""
    size = "P600_96x64"
    case = edge_case(size, "sh3")
    _, g = _gpu_run(rast, case, "colour")
    plain = fp64_reference(size, "sh3", "colour", band_grad="forward", alpha_clamp_grad="autograd")
    rel, _ = compare_grads({k: _np(v) for k, v in g.items()}, plain["grads"], case, "GPU vs fp64 (plain autograd)")
    assert {n for (k, n), v in rel.items() if v > GRAD_REL} - {"all"} == {"band_x", "band_y", "opaque"}
    assert min(rel["means3D", "band_x"], rel["means3D", "band_y"], rel["opacities", "opaque"]) > 1e-2


# ---------------------------------------------------------------- (c) the same bits by every route
ROUTE_SIZE = "P600_100x70"  # partial tiles in both directions, three 256-Gaussian blocks


@pytest.mark.parametrize("config", ["sh3", "sh0", "precomp"])
def test_backward_equals_blend_plus_preprocess(config, rast):
    case = edge_case(ROUTE_SIZE, config)
    dC = torch.tensor(loss_weights(ROUTE_SIZE)[0], device="cuda")
    st = rast.forward(case["cam"], bg=BG, **oracle_kwargs(case["inputs"]))
    one = rast.backward(st, dC)
    two = rast.backward_preprocess(st, rast.backward_blend(st, dC))
    assert one.keys() == two.keys()
    for k, v in one.items():
        assert torch.equal(v, two[k]), k


def test_recomputed_clamp_bits_equal_stored(rast):
    """B2 with the SH clamp bits it recomputes (a banded forward stores none) = B2 with the bits the full
    forward stored, where 6-9 % of the visible channels do clamp and the view is rotated."""
    case = edge_case(ROUTE_SIZE, "sh3")
    cam, dC = case["cam"], torch.tensor(loss_weights(ROUTE_SIZE)[0], device="cuda")
    assert cam.grid == (7, 5)
    for D in (3, 1):
        kw = dict(oracle_kwargs(case["inputs"]), sh_degree=D)
        st_full = rast.forward(cam, bg=BG, **kw)
        grad2d = rast.backward_blend(st_full, dC)
        stored = rast.backward_preprocess(st_full, grad2d)
        vis = st_full.radii > 0
        stopped = (stored["sh_dc"].reshape(-1, 3) == 0) & (grad2d[:, 6:9] != 0) & vis[:, None]
        share = float(stopped.sum()) / (3.0 * float(vis.sum()))  # channels whose gradient stops at the clamp
        assert share >= (0.05 if D == 3 else 0.005), (D, share)  # float64: 0.080 at degree 3, 0.008 at 1
        st_band = rast.forward(cam, bg=BG, tile_rows=(0, 4), **kw)
        recomputed = rast.backward_preprocess(st_band, grad2d)
        assert stored.keys() == recomputed.keys()
        for k, v in stored.items():
            assert torch.equal(v, recomputed[k]), (D, k)


@pytest.mark.parametrize("config", ["sh3", "precomp"])
def test_two_bands_equal_full(config, rast):
    """As test_gpu_parity.test_band_render_equals_full: each band's pixels are the full render's bit for
    bit, and B2 on the summed per-band 2D gradients gives the full backward's within 1e-5."""
    case = edge_case(ROUTE_SIZE, config)
    cam, kw = case["cam"], oracle_kwargs(case["inputs"])
    dC = torch.tensor(loss_weights(ROUTE_SIZE)[0], device="cuda")
    full = rast.forward(cam, bg=BG, **kw)
    g_full = rast.backward(full, dC)
    img, grad2d = torch.zeros_like(full.color), None
    for y0, y1 in ((0, 2), (2, cam.grid[1])):
        st = rast.forward(cam, bg=BG, tile_rows=(y0, y1), **kw)
        img[:, y0 * 16:y1 * 16] = st.color[:, y0 * 16:y1 * 16]
        g2 = rast.backward_blend(st, dC)
        grad2d = g2 if grad2d is None else grad2d + g2
    assert torch.equal(img, full.color)
    g = rast.backward_preprocess(st, grad2d)
    for k, v in g_full.items():
        assert rel_l2(_np(g[k]), _np(v)) <= 1e-5, k


@pytest.mark.parametrize("config,opacity_shape", [("sh3", "P"), ("sh3", "Px1"), ("precomp", "P")])
def test_autograd_function_equals_cabi(config, opacity_shape, rast):
    R = pkg("rasterizer")
    case = edge_case(ROUTE_SIZE, config)
    cam, kw = case["cam"], oracle_kwargs(case["inputs"])
    P = len(case["visible"])
    dC = torch.tensor(loss_weights(ROUTE_SIZE)[0], device="cuda")
    D = kw.pop("sh_degree")
    leaves = {k: torch.tensor(v, device="cuda") for k, v in kw.items() if v is not None}
    leaves["opacities"] = leaves["opacities"].reshape((P,) if opacity_shape == "P" else (P, 1))
    for v in leaves.values():
        v.requires_grad_(True)
    m2d = torch.zeros((P, 3), device="cuda", requires_grad=True)
    rest = {k: v for k, v in leaves.items() if k not in ("means3D", "opacities")}
    color, radii = R.rasterize_gaussians(cam, leaves["means3D"], m2d, leaves["opacities"], sh_degree=D, bg=BG, **rest)
    st = rast.forward(cam, bg=BG, sh_degree=D, **kw)
    assert torch.equal(st.color, color.detach()) and torch.equal(st.radii, radii)
    names = list(leaves)
    grads = torch.autograd.grad((color * dC).sum(), [leaves[k] for k in names] + [m2d])
    g = rast.backward(st, dC)
    key = dict(colors_precomp="colors", cov3D_precomp="cov3D")
    for k, got in zip(names + ["means2D"], grads):
        if k in leaves:
            assert got.shape == leaves[k].shape, k
        want = g[key.get(k, k)]
        assert torch.equal(got.reshape(want.shape), want), k


def test_batch_view_equals_single_forward(rast):
    native = pkg("native")
    case = edge_case(ROUTE_SIZE, "sh3")
    cam, kw = case["cam"], oracle_kwargs(case["inputs"])
    dC = torch.tensor(loss_weights(ROUTE_SIZE)[0], device="cuda")
    other = pkg("train_loop").look_at_camera((-2.1, -0.6, -2.7), (0.3, 0.2, 0.4), math.radians(60.0), cam.width,
                                             cam.height)
    batch = rast.forward_batch([other, cam], bg=BG, **kw)
    for c, b in zip((other, cam), batch):
        a = rast.forward(c, bg=BG, **kw)
        assert torch.equal(a.color, b.color) and torch.equal(a.radii, b.radii)
        K = a.num_rendered
        assert b.num_rendered == K and K > 0
        for what in (native.VIEW_SORTED_GID, native.VIEW_SORTED_TILE):
            assert torch.equal(a.view(what, torch.int32, K), b.view(what, torch.int32, K))
        tiles = c.grid[0] * c.grid[1]
        assert torch.equal(a.view(native.VIEW_RANGES, torch.int32, 2 * tiles), b.view(native.VIEW_RANGES, torch.int32, 2 * tiles))
        ga, gb = rast.backward(a, dC), rast.backward(b, dC)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
