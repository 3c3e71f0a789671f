"""Camera gradients on the GPU: the camera kernel against float64 (synthetic grad2d and end to end
through the dense render), determinism and the equivalence of the posed backward with the plain ones,
the translation identity against B2's own output at scale, camera tracking through render_posed and
pose refinement in the trainer.

Bars.  The camera gradient is a sum over Gaussians of terms of both signs, so every entry is compared
against the sum of the MAGNITUDES of its per-Gaussian terms (tests/pose_reference.py: the camera fields
as leaves expanded to one row per Gaussian), not against the result, which would measure the
cancellation: |got - ref| <= 1e-4 sum_g |term_g| for a given grad2d (1e-4 is the project's GRAD_REL; the
same chain evaluated in plain f32 stays within 1e-6), 2e-4 end to end (B1's own GRAD_REL on grad2d on
top).  Entries no kernel reads are exactly zero.

One deliberate difference from B2: outside the 1.3 tan(fov) guard band the forward's cx = +-limx tz, so
dJ02/dtz = fx cx / tz^3; B2 keeps upstream's in-band 2 fx cx / tz^3 there (a clamped cx taken as a
constant), the camera kernel takes the forward's own derivative -- what float64 autograd gives and what
the first test demands of its out-of-band Gaussians.  The translation identity, which compares with B2's
dL/dmeans3D, is therefore run on in-band Gaussians.
"""
import math
import warnings

import numpy as np
import pytest
import torch

import pose_reference as pr
from conftest import pkg

pytestmark = pytest.mark.gpu

CAMERA_REL, END_TO_END_REL = 1e-4, 2e-4
ZERO_ENTRIES = [3, 7, 11, 15, 18, 22, 26, 30, 35]  # viewmatrix 4k+3, projmatrix 4k+2, the pad


@pytest.fixture(scope="module")
def rast():
    return pkg("rasterizer").CAbiRasterizer("cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _forward_kwargs(inputs):
    """pose_reference's input names -> CAbiRasterizer.forward's."""
    i = inputs
    return dict(means3D=i["means"], opacities=i["opac"], scales=i.get("scales"), rotations=i.get("rots"),
                sh_dc=i.get("sh_dc"), sh_rest=i.get("sh_rest"), sh_degree=i["D"] if "colors" not in i else 0,
                colors_precomp=i.get("colors"), cov3D_precomp=i.get("cov3D"))


def _compare(got36, terms, rel, label):
    """Every one of the 36 entries against the sum of its terms; returns the worst ratio to the bar."""
    got = np.asarray(got36, np.float64)
    ref = terms.sum(0).numpy()
    scale = terms.abs().sum(0).numpy()
    err = np.abs(got - ref)
    worst = 0.0
    for e in range(36):
        bar = rel * scale[e]
        assert err[e] <= bar, (label, e, got[e], ref[e], err[e], bar)
        if scale[e] > 0:
            worst = max(worst, err[e] / scale[e])
    for e in ZERO_ENTRIES:
        assert got36[e] == 0.0 and scale[e] == 0.0, (label, e)
    return worst


CONFIGS = {"sh0": dict(D=0), "sh3": dict(D=3), "colors_precomp": dict(D=2, colors=True),
           "cov3D_precomp": dict(D=1, cov3D=True)}


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_camera_kernel_against_float64(rast, P):
    """gsr_backward_camera on a standard-normal grad2d: one block, the block edges and several
    partials in the finalize; SH degree 0 and 3, precomputed colours and covariances; anti-aliasing on
    and off; depth modes 0, 1, 2.  Culled Gaussians behind the camera and large visible ones outside
    the guard band are part of every case with enough Gaussians to hold them (make_case)."""
    worst = 0.0
    seen_band = seen_behind = 0
    for name, cfg in CONFIGS.items():
        case = pr.make_case(P, seed=P, **cfg)
        cam, vis = case["cam"], case["visible"]
        g2 = torch.as_tensor(case["grad2d"], device="cuda")
        for aa in (False, True):
            st = rast.forward(cam, antialiasing=aa, **_forward_kwargs(case["inputs"]))
            np.testing.assert_array_equal(_np(st.radii) > 0, vis)
            for mode in (0, 1, 2):
                pre = pr.preprocess(cam, antialias=aa, inverse_depth=mode == 2, **case["inputs"])
                sh_margin, band_margin = pr.margins(pre, vis)
                assert sh_margin > 1e-3 and band_margin > 1e-3, (name, sh_margin, band_margin)
                terms = pr.terms_from_grad2d(pre, case["grad2d"], vis, mode)
                got = _np(rast.backward_camera(st, g2, depth_mode=mode)["camera"])
                worst = max(worst, _compare(got, terms, CAMERA_REL, (name, P, aa, mode)))
        with torch.no_grad():
            out = (pre["txtz"].abs() > pre["limx"]) | (pre["tytz"].abs() > pre["limy"])
        seen_band += int((out.numpy() & vis).sum())
        seen_behind += int((~vis).sum())
    if P >= 255:
        assert seen_band > 0 and seen_behind > 0, (seen_band, seen_behind)
    print(f"P={P}: worst |got - ref| / sum|term| = {worst:.3e} (bar {CAMERA_REL:.0e}); "
          f"{seen_band} visible out-of-band, {seen_behind} culled")


def test_determinism_and_equivalence(rast):
    case = pr.make_case(1000, D=3, seed=11)
    cam = case["cam"]
    kw = _forward_kwargs(case["inputs"])
    rng = np.random.default_rng(12)
    dpix = rng.standard_normal((3, cam.height, cam.width)).astype(np.float32)
    dd = rng.standard_normal((cam.height, cam.width)).astype(np.float32)
    da = rng.standard_normal((cam.height, cam.width)).astype(np.float32)
    for aa in (False, True):
        st = rast.forward(cam, antialiasing=aa, **kw)
        plain = rast.backward(st, dpix)
        posed = rast.backward(st, dpix, camera_grad=True)
        again = rast.backward(st, dpix, camera_grad=True)
        assert set(posed) == set(plain) | {"camera", "viewmatrix", "projmatrix", "campos"}
        for k in plain:
            assert torch.equal(plain[k], posed[k]), k
        assert torch.equal(posed["camera"], again["camera"])
        assert posed["viewmatrix"].shape == (16,) and posed["projmatrix"].shape == (16,) and posed["campos"].shape == (3,)
        assert torch.equal(posed["camera"][:16], posed["viewmatrix"]) and torch.equal(posed["camera"][32:35], posed["campos"])
        assert float(posed["camera"].abs().max()) > 0
        # the split path: B1 + gather, then the camera pass on that grad2d
        g2 = rast.backward_blend(st, dpix)
        split = rast.backward_camera(st, g2)
        assert torch.equal(split["camera"], posed["camera"])
        assert torch.equal(rast.backward_camera(st, g2)["camera"], split["camera"])
        # the aux form
        for inv in (False, True):
            sx = rast.forward_aux(cam, antialiasing=aa, inverse_depth=inv, **kw)
            pa = rast.backward_aux(sx, dpix, dd, da)
            qa = rast.backward_aux(sx, dpix, dd, da, camera_grad=True)
            for k in pa:
                assert torch.equal(pa[k], qa[k]), (k, inv)
            assert torch.equal(qa["camera"], rast.backward_aux(sx, dpix, dd, da, camera_grad=True)["camera"])
            assert not torch.equal(qa["camera"], posed["camera"])  # the depth and alpha gradients reach the camera
    # a view of gsr_forward_batch goes through the per-view backward: its buffers give the single forward's bits
    cam2 = pkg("train_loop").look_at_camera((-2.1, -0.6, -2.7), (0.3, 0.2, 0.4), math.radians(60.0), cam.width,
                                            cam.height)
    batch = rast.forward_batch([cam, cam2], **kw)
    for c, sb in zip((cam, cam2), batch):
        single = rast.backward(rast.forward(c, **kw), dpix, camera_grad=True)
        viewed = rast.backward(sb, dpix, camera_grad=True)
        for k in single:
            assert torch.equal(single[k], viewed[k]), k
        assert torch.equal(rast.backward_camera(sb, rast.backward_blend(sb, dpix))["camera"], single["camera"])
    assert not torch.equal(rast.backward(batch[1], dpix, camera_grad=True)["camera"], posed["camera"])


def test_no_gaussians_and_all_culled_give_zeros(rast):
    cam = pr.posed_camera()
    dpix = np.ones((3, cam.height, cam.width), np.float32)
    st0 = rast.forward(cam, np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 1, 3)),
                       None, sh_degree=0)
    g = rast.backward(st0, dpix, camera_grad=True)
    assert g["camera"].shape == (36,) and float(g["camera"].abs().max()) == 0.0
    z = rast.backward_camera(st0, torch.zeros((0, 12), device="cuda"))
    assert float(z["camera"].abs().max()) == 0.0
    # every Gaussian behind the camera
    case = pr.make_case(300, D=3, seed=13)
    wv = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4)
    behind = (np.array([[0.1, -0.2, -3.0]]) + 0.3 * np.random.default_rng(14).standard_normal((300, 3)) - wv[3, :3]) \
        @ wv[:3, :3].T
    case["inputs"]["means"] = behind.astype(np.float32)
    st = rast.forward(cam, **_forward_kwargs(case["inputs"]))
    assert int((st.radii > 0).sum()) == 0
    g = rast.backward(st, dpix, camera_grad=True)
    assert float(g["camera"].abs().max()) == 0.0
    junk = torch.full((300, 12), float("nan"), device="cuda")  # the rows of culled Gaussians are never read
    assert float(rast.backward_camera(st, junk, depth_mode=1)["camera"].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["colour", "aux", "aux_inverse_antialias"])
def test_end_to_end_against_float64_dense_render(rast, mode):
    """The posed backward against float64 autograd through the dense render (dense_reference.render
    on pose_reference's expanded camera leaves): 48 x 40, 60 Gaussians, SH 2, a random dL/dcolor, and
    dL/ddepth, dL/dalpha in the aux cases."""
    cam = pr.posed_camera(48, 40)
    case = pr.make_case(60, D=2, seed=21, cam=cam)
    aux, inv, aa = mode != "colour", mode == "aux_inverse_antialias", mode == "aux_inverse_antialias"
    rng = np.random.default_rng(22)
    dC = rng.standard_normal((3, 40, 48)).astype(np.float32)
    dD = rng.standard_normal((40, 48)).astype(np.float32)
    dA = rng.standard_normal((40, 48)).astype(np.float32)
    kw = _forward_kwargs(case["inputs"])
    bg = (0.2, 0.5, 0.3)
    if aux:
        st = rast.forward_aux(cam, antialiasing=aa, inverse_depth=inv, bg=bg, **kw)
        got = rast.backward_aux(st, dC, dD, dA, camera_grad=True)
    else:
        st = rast.forward(cam, bg=bg, **kw)
        got = rast.backward(st, dC, camera_grad=True)
    np.testing.assert_array_equal(_np(st.radii) > 0, case["visible"])
    pre = pr.preprocess(cam, antialias=aa, inverse_depth=inv, **case["inputs"])
    sh_margin, band_margin = pr.margins(pre, case["visible"])
    assert sh_margin > 1e-3 and band_margin > 1e-3
    color, T, _ = pr.render(cam, pre, case["geom"], bg)
    loss = (color * torch.as_tensor(dC, dtype=torch.float64)).sum()
    if aux:
        vpre = dict(pre, rgb=torch.stack([pre["value"], torch.zeros_like(pre["value"]), torch.zeros_like(pre["value"])], 1))
        depth = pr.render(cam, vpre, case["geom"], (0.0, 0.0, 0.0))[0][0]
        loss = loss + (depth * torch.as_tensor(dD, dtype=torch.float64)).sum() + \
            ((1.0 - T) * torch.as_tensor(dA, dtype=torch.float64)).sum()
        np.testing.assert_allclose(_np(st.depth), depth.detach().numpy(), rtol=0, atol=1e-3 * float(depth.detach().abs().max()))
    np.testing.assert_allclose(_np(st.color), color.detach().numpy(), rtol=0, atol=2e-3)
    loss.backward()
    terms = pr.camera_terms(pre)
    m = torch.as_tensor(case["visible"])[:, None]
    terms = torch.where(m, terms, torch.zeros_like(terms))
    worst = _compare(_np(got["camera"]), terms, END_TO_END_REL, mode)
    print(f"{mode}: worst |got - ref| / sum|term| = {worst:.3e} (bar {END_TO_END_REL:.0e})")


def test_translation_identity_at_scale(rast):
    """Moving the camera centre by eps is moving every mean by -eps, so with G = dL/dviewmatrix +
    dL/dprojmatrix chained through full_proj = world_view @ proj, and t = G's translation row,
    -(W t) + dL/dcampos = -sum_g dL/dmeans3D[g] (W the rotation block of world_view).  100k Gaussians
    at 256 x 256: 391 block partials in the finalize, against B2's own output, no reference.  In-band
    Gaussians (see the module docstring), a tenth of them culled."""
    graphics = pkg("graphics")
    cam = pr.posed_camera(256, 256)
    P = 100_000
    rng = np.random.default_rng(31)
    wv = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4)
    z = rng.uniform(2.0, 9.0, P)
    z[::10] = rng.uniform(-4.0, 0.1, len(z[::10]))
    u = rng.uniform(-1.1, 1.1, (P, 2)) * np.array([cam.tanfovx, cam.tanfovy])
    means = ((np.stack([u[:, 0] * z, u[:, 1] * z, z], 1) - wv[3, :3]) @ wv[:3, :3].T).astype(np.float32)
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    scales = np.exp(rng.uniform(np.log(0.004), np.log(0.03), (P, 3))).astype(np.float32)
    st = rast.forward(cam, means, rng.uniform(0.1, 0.9, P).astype(np.float32), scales, q.astype(np.float32),
                      (0.5 * rng.standard_normal((P, 1, 3))).astype(np.float32),
                      (0.2 * rng.standard_normal((P, 15, 3))).astype(np.float32), sh_degree=3)
    nvis = int((st.radii > 0).sum())
    assert 0.6 * P < nvis <= 0.9 * P  # a tenth behind the camera; small ones beyond the image edge are culled too
    dpix = rng.standard_normal((3, 256, 256)).astype(np.float32)
    g = rast.backward(st, dpix, camera_grad=True)
    dV = _np(g["viewmatrix"]).astype(np.float64).reshape(4, 4)
    dP = _np(g["projmatrix"]).astype(np.float64).reshape(4, 4)
    dC = _np(g["campos"]).astype(np.float64)
    proj = graphics.get_projection_matrix(cam.znear, cam.zfar, 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)).T
    G = dV + dP @ proj.T
    lhs = -(wv[:3, :3] @ G[3, :3]) + dC
    dm = _np(g["means3D"]).astype(np.float64)
    rhs = -dm.sum(0)
    bar = 1e-4 * np.abs(dm).sum(0)
    print(f"translation identity: lhs {lhs} rhs {rhs} |diff| / sum|dmeans| {np.abs(lhs - rhs) / np.abs(dm).sum(0)}")
    assert (np.abs(lhs - rhs) <= bar).all(), (lhs, rhs, bar)
    assert (np.abs(rhs) > 10 * bar).any()  # the identity is not met by zeros


# ---------------------------------------------------------------- tracking and the trainer
def _perturbed(cam, extent, seed):
    """cam turned by 2 degrees about a random axis, its centre moved by 0.05 of the scene extent."""
    pose = pkg("pose")
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    shift = rng.standard_normal(3)
    shift *= 0.05 * extent / np.linalg.norm(shift)
    out = pose.compose(cam, np.concatenate([math.radians(2.0) * axis, shift]))
    ang, dist = pose.pose_error(out, cam)
    assert abs(ang - math.radians(2.0)) < 1e-5 and abs(dist - 0.05 * extent) < 1e-3 * extent
    return out


def _model(n, seed, gt_scale=0.08):
    TL, M = pkg("train_loop"), pkg("model")
    means, f_dc, f_rest, opac, log_s, q, _ = TL.procedural_cloud(n, seed, texture=0.0, gt_scale=gt_scale)
    m = M.GaussianModel(1)
    m.active_sh_degree = 1
    t = lambda a: torch.as_tensor(a, device="cuda")
    m._xyz, m._features_dc, m._features_rest = t(means), t(f_dc), t(f_rest)
    m._scaling, m._rotation, m._opacity = t(log_s), t(q), t(opac)
    return m


def test_tracking_with_render_posed():
    """A fixed map of 2000 Gaussians, one view, the target rendered from the true pose; the start is
    2 degrees and 0.05 of the scene extent off; Adam on delta through render_posed, at most 200 iterations."""
    R, TL, pose = pkg("rasterizer"), pkg("train_loop"), pkg("pose")
    cams = TL.orbit_cameras(4, 96, 64, seed=3)
    centres = np.stack([c.campos for c in cams]).astype(np.float64)
    extent = float(np.linalg.norm(centres - centres.mean(0), axis=1).max() * 1.1)
    true_cam = cams[1]
    model = _model(2000, 5)
    pipe, bg = R.PipelineParams(), (0.0, 0.0, 0.0)
    with torch.no_grad():
        target = R.render_posed(true_cam, torch.zeros(6, dtype=torch.float64), model, pipe, bg)["render"].clone()
    start = _perturbed(true_cam, extent, 6)
    ang0, dist0 = pose.pose_error(start, true_cam)
    delta = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([delta], lr=2e-3)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        out = R.render_posed(start, delta, model, pipe, bg)
        loss = (out["render"] - target).abs().mean()
        loss.backward()
        assert delta.grad is not None and delta.grad.dtype == torch.float64 and delta.grad.device.type == "cpu"
        losses.append(loss.detach())
        opt.step()
    with torch.no_grad():
        final = (R.render_posed(start, delta, model, pipe, bg)["render"] - target).abs().mean()
    ang1, dist1 = pose.pose_error(pose.compose(start, delta.detach()), true_cam)
    first = float(losses[0])
    print(f"tracking: rotation {math.degrees(ang0):.3f} -> {math.degrees(ang1):.3f} deg (ratio {ang1 / ang0:.3f}), "
          f"centre {dist0:.4f} -> {dist1:.4f} (ratio {dist1 / dist0:.3f}), loss {first:.5f} -> {float(final):.5f}")
    assert ang1 < 0.5 * ang0 and dist1 < 0.5 * dist0
    assert float(final) < first


def _pose_trainer(scene, opt, seed=0):
    T = pkg("trainer")
    tr = T.GaussianTrainer.from_point_cloud(scene.points, scene.colors, 1, spatial_lr_scale=scene.extent, opt=opt,
                                            device="cuda", seed=seed)
    if opt.train_poses:
        tr.setup_poses(len(scene.cams))
    return tr


@pytest.fixture(scope="module")
def pose_scene():
    TL = pkg("train_loop")
    scene = TL.synthetic_scene(3000, 3000, 8, 96, 64, seed=4, texture=0.0, gt_scale=0.05)
    noisy = [_perturbed(c, scene.extent, 40 + i) for i, c in enumerate(scene.cams)]
    return scene, noisy


def _run(tr, scene, noisy, first, last):
    for it in range(first, last + 1):
        v = (it - 1) % len(noisy)
        tr.step(it, noisy[v], scene.gts[v], densify=False, view_index=v)


def _mean_error(cams, true_cams):
    pose = pkg("pose")
    e = np.array([pose.pose_error(a, b) for a, b in zip(cams, true_cams)])
    return e.mean(0)


def test_trainer_refines_poses(pose_scene):
    T = pkg("trainer")
    scene, noisy = pose_scene
    opt = T.OptimizationParams(iterations=400, position_lr_max_steps=400, train_poses=True, pose_lr_init=1e-3,
                               pose_lr_final=1e-4)
    tr = _pose_trainer(scene, opt)
    start = _mean_error(tr.refined_cameras(noisy), scene.cams)
    np.testing.assert_allclose(start, _mean_error(noisy, scene.cams), rtol=0, atol=0)
    _run(tr, scene, noisy, 1, 320)
    end = _mean_error(tr.refined_cameras(noisy), scene.cams)
    print(f"trainer: mean rotation error {math.degrees(start[0]):.3f} -> {math.degrees(end[0]):.3f} deg, "
          f"mean centre error {start[1]:.4f} -> {end[1]:.4f}; {tr.pose_updates_dropped} updates dropped")
    assert end[0] < start[0] and end[1] < start[1]
    # the centre error carries the margin (measured 0.72 of its start): a wrong sign in either half of the
    # chain moves the centres away, not a tenth closer
    assert end[1] < 0.9 * start[1]
    assert tr.poses.steps.tolist() == [40] * 8 and tr.pose_updates_dropped == 0
    assert not tr._pose_pending


def test_trainer_runs_do_not_depend_on_timing(pose_scene):
    T = pkg("trainer")
    scene, noisy = pose_scene
    opt = T.OptimizationParams(iterations=400, position_lr_max_steps=400, train_poses=True, pose_lr_init=1e-3)
    deltas = []
    for rep in range(2):
        tr = _pose_trainer(scene, opt)
        for it in range(1, 41):
            v = (it - 1) % 8
            tr.step(it, noisy[v], scene.gts[v], densify=False, view_index=v)
            if rep == 1 and it % 7 == 0:
                torch.cuda.synchronize()  # a different host / device interleaving
        tr.flush_poses()
        deltas.append(tr.poses.delta.copy())
    assert deltas[0].tobytes() == deltas[1].tobytes()
    assert np.abs(deltas[0]).max() > 0


def test_first_posed_step_is_the_plain_step(pose_scene):
    """With every delta zero the composed camera is the camera bit for bit and gsr_backward_posed
    writes gsr_backward's leaf gradients: the first step leaves the same model behind."""
    T = pkg("trainer")
    scene, noisy = pose_scene
    out = []
    for posed in (False, True):
        opt = T.OptimizationParams(iterations=400, position_lr_max_steps=400, train_poses=posed)
        tr = _pose_trainer(scene, opt)
        o = tr.step(1, noisy[2], scene.gts[2], densify=False, view_index=2 if posed else None)
        out.append((o, {k: v.clone() for k, v in tr.params.items()}, {k: v.clone() for k, v in tr.exp_avg.items()}))
    assert torch.equal(out[0][0]["image"], out[1][0]["image"])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
        assert torch.equal(out[0][2][k], out[1][2][k]), k
    assert "dL_dcamera" in out[1][0] and "dL_dcamera" not in out[0][0]
    assert float(out[1][0]["dL_dcamera"].abs().max()) > 0


def test_overflowed_render_drops_its_pose_update(pose_scene):
    T = pkg("trainer")
    scene, noisy = pose_scene
    opt = T.OptimizationParams(iterations=400, position_lr_max_steps=400, train_poses=True, pose_lr_init=1e-3)
    tr = _pose_trainer(scene, opt)
    _run(tr, scene, noisy, 1, 8)
    tr.flush_poses()
    assert tr.binning.cap > 0 and tr.pose_updates_dropped == 0
    before = tr.poses.delta.copy()
    steps = tr.poses.steps.copy()
    k = tr.binning.k_max
    tr.binning.cap = max(16, k // 4)  # the next render's bound is far below its K
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr.step(9, noisy[0], scene.gts[0], densify=False, view_index=0)
        tr.flush_poses()
        torch.cuda.synchronize()
        tr.binning.poll()
    assert tr.pose_updates_dropped == 1 and tr.binning.overflows == 1
    assert tr.poses.delta.tobytes() == before.tobytes() and tr.poses.steps.tolist() == steps.tolist()
    tr.step(10, noisy[1], scene.gts[1], densify=False, view_index=1)  # sized exactly again: applied
    tr.flush_poses()
    assert tr.poses.steps[1] == steps[1] + 1 and tr.pose_updates_dropped == 1


def test_capture_restore_continues_identically(pose_scene, tmp_path):
    T = pkg("trainer")
    scene, noisy = pose_scene
    opt = T.OptimizationParams(iterations=400, position_lr_max_steps=400, train_poses=True, pose_lr_init=1e-3)
    a = _pose_trainer(scene, opt)
    _run(a, scene, noisy, 1, 20)
    path = str(tmp_path / "mid.ckpt")
    a.capture(path)
    assert not a._pose_pending  # capture flushes
    _run(a, scene, noisy, 21, 40)
    a.flush_poses()
    b = _pose_trainer(scene, opt)
    b.restore(path)
    assert b.poses is not None and b.poses.steps.sum() == 20
    _run(b, scene, noisy, 21, 40)
    b.flush_poses()
    for name in ("delta", "exp_avg", "exp_avg_sq", "steps"):
        assert getattr(a.poses, name).tobytes() == getattr(b.poses, name).tobytes(), name
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
    # a checkpoint without poses restores as before
    plain = _pose_trainer(scene, T.OptimizationParams(iterations=400, position_lr_max_steps=400))
    plain.step(1, scene.cams[0], scene.gts[0], densify=False)
    p2 = str(tmp_path / "plain.ckpt")
    plain.capture(p2)
    b.restore(p2)
    assert b.poses is None
