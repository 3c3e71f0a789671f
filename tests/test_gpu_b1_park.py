"""B1's deferred reduction (csrc/gsr_blend.hip: park / park_flush and the wave-uniform contributor
flag) at the smallest shapes that reach every path of it.

A record's quad partials wait in LDS and are flushed every PARK contributing records, or at the
end of a 64-record batch.  The count sweep puts N Gaussians that all cover one tile (low opacity,
so no pixel finishes) at the counts around the parking depth and the batch size: a full flush, a
partial flush at a batch end, a flush that ends exactly at a batch end, several batches.  A 32x32
image (4 tiles) takes the band instantiations (prefetching B1, four-wave F6), a 1024x1024 image
(4096 tiles) the full-image ones; the depth / alpha entry points repeat the sweep with the tenth
moment.  The finished-stripe scene has records that B1 visits (or culls) without a contribution:
they must stay exactly zero while their neighbours in the list are parked and flushed.

Bars: the parity suite's, as they are (GRAD_REL, ELEM_GRAD, GRAD_FLIPS of tests/test_gpu_parity.py)
against the CPU oracle, and two backward calls on one state bitwise equal.
"""
import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2
from test_gpu_parity import ELEM_GRAD, GRAD_FLIPS, GRAD_KEYS, GRAD_REL, elementwise_misses
from test_native_aux import aux_reference, make_aux_grads

pytestmark = pytest.mark.gpu

PARK = 4  # kPark of csrc/gsr_blend.hip (not exported through the C ABI)
COUNTS = sorted({1, PARK - 1, PARK, PARK + 1, 2 * PARK - 1, 2 * PARK, 63, 64, 65, 64 + PARK + 1, 130})
AUX_KEYS = GRAD_KEYS + ["conic"]
# (W, H, the tile the Gaussians sit on): 4 tiles -> band forms, 4096 tiles -> full-image forms
SIZES = {"band": (32, 32, (0, 1)), "full": (1024, 1024, (31, 33))}


@pytest.fixture(scope="module")
def rast():
    return pkg("rasterizer").CAbiRasterizer("cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _world(cam, cx, cy, z):
    """World position whose projection is the centre of pixel (cx, cy) at depth z (R = I, T = 0)."""
    x = ((2.0 * cx + 1.0) / cam.width - 1.0) * cam.tanfovx * z
    y = ((2.0 * cy + 1.0) / cam.height - 1.0) * cam.tanfovy * z
    return np.stack([x, y, z], 1)


def _covering(cam, tile, N, rng, z0=3.0, dz=0.02):
    """N Gaussians of sigma 20 - 28 px centred within 3 px of the tile's centre, opacity 0.02 - 0.03: on
    the tile every alpha is above 0.015 (far from the 1 / 255 cut) and after 130 of them T stays
    above 0.02 (far from the 1e-4 cut)."""
    fx = cam.width / (2.0 * cam.tanfovx)
    cx = 16 * tile[0] + 7.5 + rng.uniform(-3.0, 3.0, N)
    cy = 16 * tile[1] + 7.5 + rng.uniform(-3.0, 3.0, N)
    z = z0 + dz * np.arange(N)
    s = (24.0 * z / fx)[:, None] * rng.uniform(0.85, 1.15, (N, 3))  # anisotropic: rotations matter
    q = rng.normal(0.0, 1.0, (N, 4))
    return dict(means3D=_world(cam, cx, cy, z), scales=s, opacities=rng.uniform(0.02, 0.03, (N, 1)),
                rotations=q / np.linalg.norm(q, axis=1, keepdims=True))


def _finish(parts, rng):
    """Concatenate the parts (in gid order; identity rotations where a part has none) and add random
    SH1 colours."""
    ident = lambda p: np.tile(np.array([[1.0, 0.0, 0.0, 0.0]]), (len(p["means3D"]), 1))
    parts = [dict(p, rotations=p.get("rotations", ident(p))) for p in parts]
    cat = {k: np.concatenate([p[k] for p in parts]).astype(np.float32)
           for k in ("means3D", "scales", "opacities", "rotations")}
    P = len(cat["means3D"])
    cat["sh_dc"] = rng.normal(0.0, 0.3, (P, 1, 3)).astype(np.float32)
    cat["sh_rest"] = rng.normal(0.0, 0.05, (P, 3, 3)).astype(np.float32)
    return cat


def _count_scene(size, N):
    W, H, tile = SIZES[size]
    cam = pkg("graphics").synthetic_camera(W, H)
    rng = np.random.default_rng(1000 + N)
    inputs = _finish([_covering(cam, tile, N, rng)], rng)
    return cam, inputs, pkg("scene").make_dL_dpix(cam, seed=N)


def _check(g_gpu, g_cpu, keys):
    worst = {}
    for k in keys:
        if k in g_gpu:
            want = g_cpu[k]
            a = _np(g_gpu[k]).reshape(want.shape)
            r = rel_l2(a, want)
            worst[k] = elementwise_misses(a, want, *ELEM_GRAD)
            print(f"grad {k}: rel_l2 {r:.3e} misses {worst[k][0]:.3e}")
            assert r <= GRAD_REL, (k, r)
    assert worst and max(v[0] for v in worst.values()) <= GRAD_FLIPS, worst


def _bitwise(ga, gb):
    assert ga.keys() == gb.keys()
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("size", list(SIZES))
def test_count_sweep(size, N, rast, oracle):
    cam, inputs, dpix = _count_scene(size, N)
    st = rast.forward(cam, **inputs, sh_degree=1)
    f = oracle.forward(cam, **inputs, sh_degree=1)
    assert st.num_rendered == f.num_rendered
    # every Gaussian is in the tile's list, so B1 sees N records there
    tx, ty = SIZES[size][2]
    r0, r1 = f.state.ranges()[ty * cam.grid[0] + tx]
    assert int(r1) - int(r0) == N
    g = rast.backward(st, dpix)
    _check(g, f.state.backward(dpix), GRAD_KEYS)
    _bitwise(g, rast.backward(st, dpix))


@pytest.mark.parametrize("N", COUNTS)
def test_count_sweep_aux(N, rast, oracle):
    """The sweep through gsr_forward_aux / gsr_backward_aux (tenth moment, its own parking bound)."""
    cam, inputs, dC = _count_scene("band", N)
    dD, dA = make_aux_grads(cam, seed=N + 1)
    st = rast.forward_aux(cam, **inputs, sh_degree=1)
    ref = aux_reference(oracle, cam, inputs, 1, dC, dD, dA)
    assert st.num_rendered == ref["num_rendered"]
    g = rast.backward_aux(st, dC, dD, dA)
    _check(g, ref["grads"], AUX_KEYS)
    _bitwise(g, rast.backward_aux(st, dC, dD, dA))


@pytest.mark.parametrize("size", list(SIZES))
def test_finished_stripes_contribute_nothing(size, rast, oracle):
    """16 sheets of alpha 0.98 (sigma 40 x 3 px on tile row 3.5) finish every pixel of the tile's two
    upper stripes (alpha >= 0.49 per sheet there: T < 1e-4 after 14) and leave the lowest stripe
    live (alpha < 0.02 at rows 12 and below).  Behind them, interleaved in depth: 24 small opaque
    Gaussians (sigma 0.8 px, footprint inside the finished rows) and 20 of the count sweep's
    covering ones.  The small ones get exactly zero gradients -- whether B1 culls them by the
    stripe masks or visits them on stale live bits -- while the covering ones, parked and flushed
    around them, and the sheets match the oracle."""
    W, H, tile = SIZES[size]
    cam = pkg("graphics").synthetic_camera(W, H)
    rng = np.random.default_rng(7)
    fx = cam.width / (2.0 * cam.tanfovx)
    L, M, N = 16, 24, 20
    zs = 1.2 + 0.02 * np.arange(L)
    sheets = dict(means3D=_world(cam, np.full(L, 16 * tile[0] + 7.5), np.full(L, 16 * tile[1] + 3.5), zs),
                  scales=np.stack([40.0 * zs / fx, 3.0 * zs / fx, 3.0 * zs / fx], 1),
                  opacities=np.full((L, 1), 0.98))
    zm = 3.0 + 0.04 * np.arange(M)
    small = dict(means3D=_world(cam, 16 * tile[0] + rng.uniform(3.0, 12.0, M),
                                16 * tile[1] + 3.5 + rng.uniform(-0.5, 0.5, M), zm),
                 scales=np.tile((0.8 * zm / fx)[:, None], (1, 3)), opacities=np.full((M, 1), 0.9))
    cover = _covering(cam, tile, N, rng, z0=3.02, dz=0.04)
    inputs = _finish([sheets, small, cover], rng)
    dpix = pkg("scene").make_dL_dpix(cam, seed=8)
    st = rast.forward(cam, **inputs, sh_degree=1)
    f = oracle.forward(cam, **inputs, sh_degree=1)
    assert st.num_rendered == f.num_rendered
    assert np.all(f.radii[L:L + M] > 0)  # the small ones are in the lists
    g = rast.backward(st, dpix)
    g_cpu = f.state.backward(dpix)
    behind = slice(L, L + M)
    for k in GRAD_KEYS:
        if k in g:
            # the scene does what it says: the oracle gives the small ones nothing either
            assert not np.any(g_cpu[k][behind]), k
            assert not np.any(_np(g[k]).reshape(g_cpu[k].shape)[behind]), k
    # the covering ones still contribute (on the live stripes)
    assert np.all(np.abs(g_cpu["opacities"][L + M:]).reshape(N, -1).max(1) > 0)
    _check(g, g_cpu, GRAD_KEYS)
    _bitwise(g, rast.backward(st, dpix))
