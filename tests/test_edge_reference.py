"""The edge scene and its float64 reference, pinned on the CPU (no GPU needed).

The edge scene (pose_reference.make_case(edge=True)) is a posed camera -- no zero among the nine
rotation entries of its view matrix -- over Gaussians on every branch the easy scenes never reach:
centres outside the 1.3 tan(fov) guard band in x and in y, behind the camera, just inside and just
outside the 0.2 near plane, opacities that saturate alpha at 0.99 and pixels that terminate on
T < 1e-4, SH colour sums on both sides of the clamp at 0, precomputed colours and covariances.

The reference is float64 autograd through pose_reference.preprocess and dense_reference.render with
the kernels' two conventions switched on: band_grad="upstream" (a clamped cx, cy is a
constant) and alpha_clamp_grad="upstream" (the gradient passes straight through min(0.99, o G)).
Here the f32 CPU oracle is held against it -- all rows and every class of rows on its own -- and
against the plain-autograd forms, from which it must differ on exactly the out-of-band and opaque
classes.  tests/test_gpu_edges.py holds the HIP kernels against both.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import pose_reference as pr
from conftest import rel_l2
from test_gpu_parity import ELEM_GRAD, GRAD_REL, RGB_REL, elementwise_misses

DT = torch.float64
BG = (0.2, 0.5, 0.3)
MODES = ("colour", "aux", "aux_inverse_antialias")
CONFIGS = {"sh3": dict(D=3), "sh0": dict(D=0), "precomp": dict(D=0, colors=True, cov3D=True)}
# (P, W, H, fovx in degrees).  The small image takes a narrower field of view: at 60 degrees its footprints
# are a quarter of the larger images' in pixels and under 0.5 % of its pixels terminate
SIZES = {"P600_96x64": (600, 96, 64, 60.0), "P600_100x70": (600, 100, 70, 60.0), "P257_48x40": (257, 48, 40, 30.0)}
# make_case seeds per size, chosen on the CPU alone from 1 .. 6: every configuration meets every condition
# of check_conditions, and the two CPU references (the f32 oracle, float64) agree on it within the bars of
# test_oracle_against_fp64_with_conventions.  Not every seed does: at 257 Gaussians one cancelling element
# of a near-plane row is often outside ELEM_GRAD (seeds 1, 3, 4, 5, 6), and P600_100x70 seed 6 has a
# (pixel, Gaussian) pair on the alpha >= 1/255 cut that the two decide differently (rotations 2.9e-4)
SEEDS = {"P600_96x64": 1, "P600_100x70": 2, "P257_48x40": 2}
CASES = [(s, c) for s in SIZES for c in CONFIGS]
# reference leaf name -> gradient key of the rasterizers and the oracle
LEAVES = dict(means="means3D", opac="opacities", scales="scales", rots="rotations", sh_dc="sh_dc", sh_rest="sh_rest",
              colors="colors", cov3D="cov3D")


@functools.lru_cache(maxsize=None)
def edge_case(size, config):
    P, W, H, fov = SIZES[size]
    case = pr.make_case(P, seed=SEEDS[size], cam=pr.rolled_camera(W, H, fov), edge=True, **CONFIGS[config])
    case["size"], case["config"] = size, config
    return case


def oracle_kwargs(inputs):
    """pose_reference's input names -> the oracle's and CAbiRasterizer.forward's."""
    i = inputs
    return dict(means3D=i["means"], opacities=i["opac"], scales=i.get("scales"), rotations=i.get("rots"),
                sh_dc=i.get("sh_dc"), sh_rest=i.get("sh_rest"), sh_degree=i["D"] if "colors" not in i else 0,
                colors_precomp=i.get("colors"), cov3D_precomp=i.get("cov3D"))


@functools.lru_cache(maxsize=None)
def loss_weights(size):
    """Random dL/dcolor (3, H, W), dL/ddepth and dL/dalpha (H, W) of one image size, f32."""
    P, W, H, _ = SIZES[size]
    rng = np.random.default_rng(7000 + W)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(3, H, W), f(H, W), f(H, W)


@functools.lru_cache(maxsize=None)
def fp64_reference(size, config, mode="colour", band_grad="upstream", alpha_clamp_grad="upstream"):
    """Images and leaf gradients of the edge case in float64: dict(color, depth, alpha, T, last, pre,
    grads).  grads: the rasterizers' keys, "means2D" the (P, 2) gradient of the NDC centre; rows of
    culled Gaussians are zero.  The loss is sum(color dC) (+ sum(depth dD) + sum(alpha dA) in the aux
    modes, composed as test_gpu_camera_grad's end-to-end case composes them)."""
    assert mode in MODES
    case = edge_case(size, config)
    cam, inp = case["cam"], case["inputs"]
    aux, inv = mode != "colour", mode == "aux_inverse_antialias"
    dC, dD, dA = (torch.as_tensor(a, dtype=DT) for a in loss_weights(size))
    leaves = {k: torch.tensor(v, dtype=DT, requires_grad=True) for k, v in inp.items() if k != "D"}
    pre = pr.preprocess(cam, D=inp["D"], antialias=inv, inverse_depth=inv, band_grad=band_grad, **leaves)
    pre["ndc"].retain_grad()
    color, T, last = pr.render(cam, pre, case["geom"], BG, alpha_clamp_grad=alpha_clamp_grad)
    loss = (color * dC).sum()
    out = dict(color=color.detach().numpy(), T=T.detach().numpy(), last=last.numpy(), pre=pre)
    if aux:
        v = pre["value"]
        vpre = dict(pre, rgb=torch.stack([v, torch.zeros_like(v), torch.zeros_like(v)], 1))
        depth = pr.render(cam, vpre, case["geom"], (0.0, 0.0, 0.0), alpha_clamp_grad=alpha_clamp_grad)[0][0]
        loss = loss + (depth * dD).sum() + ((1.0 - T) * dA).sum()
        out.update(depth=depth.detach().numpy(), alpha=1.0 - out["T"])
    loss.backward()
    vis = case["visible"]
    grads = {"means2D": pre["ndc"].grad.numpy()}
    for k, t in leaves.items():
        grads[LEAVES[k]] = np.zeros(t.shape) if t.grad is None else t.grad.numpy()
    for k, g in grads.items():
        assert np.isfinite(g[vis]).all(), k
        g[~vis] = 0.0  # nothing of a culled Gaussian reaches the loss
    out["grads"] = grads
    return out


def class_rows(case):
    """name -> row mask of the visible members, "all" first, then every class that has any."""
    vis = case["visible"]
    rows = {"all": vis.copy()}
    for name in pr.EDGE_VISIBLE:
        m = case["classes"][name] & vis
        if m.any():
            rows[name] = m
    return rows


def compare_grads(got, ref, case, label, bar=GRAD_REL):
    """Every gradient tensor of `got` (the rasterizers' keys; means2D by its first two columns) against
    `ref` over all visible rows and over each class's rows.  Prints the table; returns
    {(key, class): rel-L2}, {key: fraction outside ELEM_GRAD over all rows} for the caller to assert."""
    rows = class_rows(case)
    rel, miss = {}, {}
    print(f"\n{label}: rel-L2 per tensor and class of rows (bar {bar:.0e})")
    print(f"{'':>10}" + "".join(f"{n:>10}" for n in rows) + f"{'elem-miss':>11}")
    for k, want in ref.items():
        if k not in got:
            continue
        P = want.shape[0]
        a = np.asarray(got[k], np.float64).reshape(P, -1)
        b = want.reshape(P, -1)
        if k == "means2D":
            a = a[:, :2]
        if not np.abs(b).max() > 0:
            assert not np.abs(a).max() > 0, k  # e.g. sh_rest at degree 0: zero on both sides
            continue
        for n, m in rows.items():
            rel[k, n] = rel_l2(a[m], b[m])
        miss[k] = elementwise_misses(a, b, *ELEM_GRAD)[0]
        print(f"{k:>10}" + "".join(f"{rel[k, n]:>10.2e}" for n in rows) + f"{miss[k]:>11.2e}")
    return rel, miss


def oracle_run(oracle, case):
    f = oracle.forward(case["cam"], bg=BG, **oracle_kwargs(case["inputs"]))
    return f, f.state.backward(loss_weights(case["size"])[0])


def check_conditions(case, oracle):
    """What keeps a test on this case from being vacuous or from sitting on a branch edge.  Conditions
    on the inputs, not tolerances: a seed that misses one is replaced, the condition stays."""
    cam, inp, vis, cls = case["cam"], case["inputs"], case["visible"], case["classes"]
    # a posed camera: no zero among the rotation entries, so a transposed V[4k+i] cannot go unseen
    rot = np.asarray(cam.viewmatrix, np.float64)[[0, 1, 2, 4, 5, 6, 8, 9, 10]]
    assert np.abs(rot).min() > 0.1, rot
    for name in pr.EDGE_VISIBLE:
        n = int((cls[name] & vis).sum())
        assert n >= 10, (name, n)
    for name in pr.EDGE_CULLED:
        assert cls[name].any() and not (cls[name] & vis).any(), name
    tz = case["geom"]["depth"].numpy()
    assert tz.dtype == np.float32 and np.abs(tz - np.float32(0.2)).min() >= 0.01
    assert (tz[cls["near_out"]] > 0).all() and (tz[cls["behind"]] <= 0).all()  # two different culls
    ref = fp64_reference(case["size"], case["config"])
    pre = ref["pre"]
    sh_margin, band_margin = pr.margins(pre, vis)
    assert sh_margin > 1e-3 and band_margin > 1e-3, (sh_margin, band_margin)
    with torch.no_grad():
        out_x = (pre["txtz"].abs() > pre["limx"]).numpy()
        out_y = (pre["tytz"].abs() > pre["limy"]).numpy()
    np.testing.assert_array_equal(out_x, cls["band_x"])
    assert (out_y[cls["band_y"]]).all() and not out_y[vis & ~cls["band_y"]].any()
    stats = {}
    if pre["sh_sum"] is not None:
        stats["clamped SH channels"] = float((pre["sh_sum"].detach().numpy()[vis] < 0).mean())
        # at degree 0 the colour is 0.28 dc + 0.5 and clamps 3.5 sigma out: that case is run against the
        # oracle for its kernels' instantiation, the clamp is the degree-3 cases' to cover
        assert stats["clamped SH channels"] >= 0.05 or inp["D"] == 0, stats
    f = oracle.forward(cam, bg=BG, **oracle_kwargs(inp))
    np.testing.assert_array_equal(f.radii > 0, vis)
    T, n = f.state.pixel_state()
    stats["pixels ending T < 1e-3"] = float((T < 1e-3).mean())
    assert stats["pixels ending T < 1e-3"] >= 0.03, stats
    np.testing.assert_array_equal(n.astype(np.int64), ref["last"])
    # alpha does saturate: around an opaque centre o G > 0.99 at the nearest pixel centre for some
    with torch.no_grad():
        d = pre["xy"] - torch.floor(pre["xy"] + 0.5)
        co = pre["conic"]
        peak = pre["opacity"] * torch.exp(-0.5 * (co[:, 0] * d[:, 0] ** 2 + co[:, 2] * d[:, 1] ** 2) - co[:, 1] * d[:, 0] * d[:, 1])
    stats["opaque rows with o G > 0.99 at a pixel"] = int((peak.numpy()[cls["opaque"] & vis] > 0.99).sum())
    assert stats["opaque rows with o G > 0.99 at a pixel"] >= 10, stats
    return stats


def _digest(case):
    h = hashlib.sha256()
    for k in sorted(case["inputs"]):
        v = case["inputs"][k]
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes() if hasattr(v, "tobytes") else repr(v).encode())
    h.update(case["grad2d"].tobytes())
    h.update(case["visible"].tobytes())
    return h.hexdigest()[:16]


def test_default_make_case_is_unchanged():
    """The camera tests' cases: make_case without the edge option draws what it drew before the option
    existed (digest of inputs, grad2d and visible of make_case(257, seed=257), taken at that commit)."""
    assert _digest(pr.make_case(257, seed=257)) == "4d7ff02c4d6d5b6e"
    with pytest.raises(ValueError):
        pr.preprocess(pr.posed_camera(), np.zeros((1, 3)), np.ones(1), colors=np.ones((1, 3)), cov3D=np.ones((1, 6)),
                      band_grad="autograd")


@pytest.mark.parametrize("size,config", CASES)
def test_edge_case_conditions(size, config, oracle):
    stats = check_conditions(edge_case(size, config), oracle)
    case = edge_case(size, config)
    counts = {n: int((case["classes"][n] & case["visible"]).sum()) for n in pr.EDGE_VISIBLE}
    print(f"\n{size} {config}: visible per class {counts}; " + "; ".join(f"{k} {v:.3f}" for k, v in stats.items()))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("config", ["sh3", "precomp"])
def test_oracle_against_fp64_with_conventions(size, config, oracle):
    """The f32 oracle against float64 with the kernels' conventions: radii and contributor counts equal,
    image rel-L2 <= RGB_REL, every gradient tensor rel-L2 <= GRAD_REL over all rows and over each
    class's rows, no value outside ELEM_GRAD.  Measured worst rel-L2 over the three sizes: SH 3.0e-5
    (means2D, the near-plane rows; 2.4e-5 over all rows, means3D), precomputed 1.7e-5 (cov3D, the
    near-plane rows); every other class <= 8.7e-6; image <= 7.9e-7, max abs 1.0e-5."""
    case = edge_case(size, config)
    ref = fp64_reference(size, config)
    f, g = oracle_run(oracle, case)
    np.testing.assert_array_equal(f.radii, case["geom"]["radius"].numpy())
    np.testing.assert_array_equal(f.state.pixel_state()[1].astype(np.int64), ref["last"])
    r = rel_l2(f.color, ref["color"])
    print(f"\n{size} {config}: image rel-L2 {r:.2e}, max abs {np.abs(f.color - ref['color']).max():.2e}")
    assert r <= RGB_REL
    rel, miss = compare_grads(g, ref["grads"], case, f"oracle vs fp64 (upstream conventions), {size} {config}")
    assert max(rel.values()) <= GRAD_REL, max(rel.items(), key=lambda kv: kv[1])
    assert max(miss.values()) == 0.0, miss
    for k, v in g.items():
        assert not v[~case["visible"]].any(), k


@pytest.mark.parametrize("size", list(SIZES))
def test_plain_autograd_is_the_wrong_reference(size, oracle):
    """Non-vacuity: with either switch at its plain-autograd form the oracle differs from float64 by more
    than 1e-2 on the rows of the class the switch concerns -- means3D of each out-of-band class,
    opacities of the opaque class -- and on no other class of rows (every other class stays within
    GRAD_REL).  So a kernel on the other side of a convention fails the 1e-4 bar by two orders of
    magnitude, and a test against plain autograd fails with a correct kernel.  Measured at the three
    sizes: band_x >= 3.3e-2, band_y >= 1.9e-2, opaque >= 5.5e-2."""
    case = edge_case(size, "sh3")
    f, g = oracle_run(oracle, case)
    plain = fp64_reference(size, "sh3", band_grad="forward", alpha_clamp_grad="autograd")
    rel, _ = compare_grads(g, plain["grads"], case, f"oracle vs fp64 (plain autograd), {size}")
    assert rel["means3D", "band_x"] > 1e-2 and rel["means3D", "band_y"] > 1e-2 and rel["opacities", "opaque"] > 1e-2
    assert np.abs(plain["color"] - fp64_reference(size, "sh3")["color"]).max() < 1e-12  # the values do not move
    failing = {n for (k, n), v in rel.items() if v > GRAD_REL} - {"all"}
    assert failing == {"band_x", "band_y", "opaque"}, failing  # exactly these classes, no other
    # one switch at a time.  The band switch moves the out-of-band rows' means3D alone (B2 is per Gaussian);
    # over all rows that can stay under the bar (9.9e-5 at 257 Gaussians), which is why the classes are
    # compared on their own
    band = fp64_reference(size, "sh3", band_grad="forward")
    rel, _ = compare_grads(g, band["grads"], case, f"oracle vs fp64 (band_grad forward only), {size}")
    assert {n for (k, n), v in rel.items() if v > GRAD_REL} - {"all"} == {"band_x", "band_y"}
    assert {k for (k, n), v in rel.items() if v > GRAD_REL} == {"means3D"}
    # the alpha switch moves the opaque rows alone: a saturated Gaussian's own gradient is what the clamp's
    # derivative removes
    alpha = fp64_reference(size, "sh3", alpha_clamp_grad="autograd")
    rel, _ = compare_grads(g, alpha["grads"], case, f"oracle vs fp64 (alpha_clamp_grad autograd only), {size}")
    assert {n for (k, n), v in rel.items() if v > GRAD_REL} - {"all"} == {"opaque"}
    assert rel["opacities", "opaque"] > 1e-2
