"""Camera gradients and pose refinement without a GPU: the new ABI symbols (declared, listed, exported,
scratch sizing, every refusal before a device call), the pose module against closed forms and float64
central differences, and the trainer's pose options and checkpoint state."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

HEADER = os.path.join(ROOT, "include", "gsr", "gsr.h")
NEW = ["gsr_camera_grad_scratch_bytes", "gsr_backward_camera", "gsr_backward_posed"]


def _camera():
    return pkg("train_loop").look_at_camera((1.7, -0.9, -3.1), (0.3, 0.2, 0.4), math.radians(60.0), 96, 64)


def test_symbols_declared_listed_and_exported():
    native = pkg("native")
    text = open(HEADER).read()
    for f in NEW:
        assert re.search(rf"^\s*(?:size_t|int)\s+{f}\s*\(", text, re.M), f
        assert f in native.EXPORTS
    assert int(re.search(r"#define GSR_CAMERA_GRAD_FLOATS (\d+)", text).group(1)) == native.CAMERA_GRAD_FLOATS == 36
    out = subprocess.run(["nm", "-D", "--defined-only", native.hip_library_path()], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW if f not in syms]
    assert native.load_hip().gsr_abi_version() == native.ABI_VERSION == 4  # new symbols only
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", text).group(1)) == 4


def test_scratch_bytes_positive_and_monotone():
    L = pkg("native").load_hip()
    ps = [0, 1, 255, 256, 257, 1000, 100_000, 1_000_000, 2**31 - 1]
    sizes = [int(L.gsr_camera_grad_scratch_bytes(p)) for p in ps]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[1] < sizes[-1]
    # one 27-float partial per block of 256 Gaussians
    assert sizes[5] >= 4 * 27 * 4 and sizes[7] <= (1_000_000 // 256 + 2) * 27 * 4


def _fake_call():
    """Arguments of a well-formed call over fake pointers (never dereferenced: the checks come first)."""
    native = pkg("native")
    text = open(HEADER).read()
    TAG = int(re.search(r"#define GSR_LAYOUT_TAG (0x[0-9A-Fa-f]+)u?", text).group(1), 0)
    RB = int(re.search(r"#define GSR_LAYOUT_ROW_BUCKETED (\d+)u?", text).group(1))
    c = native.Camera()
    c.width, c.height = 64, 48
    g = native.Gaussians()
    g.P, g.sh_degree = 5, 0
    fake = ctypes.c_void_p(1 << 20)
    g.means3D = g.opacities = g.sh_dc = g.scales = g.rotations = fake
    s = native.Settings()
    s.tile_y1 = 2**31 - 1
    gr = native.Grads()
    gr.dL_dmeans2D = gr.dL_dopacity = gr.dL_dmeans3D = gr.dL_dsh_dc = gr.dL_dscales = gr.dL_drotations = fake
    b = native.Buffers()
    b.geom = b.binning = b.image = fake
    # a 4 x 3-tile image of 5 Gaussians takes the row-bucketed binning (test_native_abi)
    b.n_local, b.capacity, b.num_rendered, b.layout = 5, 64, 64, TAG | RB
    return native, c, g, s, gr, b, fake


def test_refusals_come_before_any_device_call():
    native, c, g, s, gr, b, fake = _fake_call()
    L = native.load_hip()
    err_layout = native.GSR_ERR_LAYOUT
    calls = []
    alloc = native.ALLOC_FN(lambda _c, n: calls.append(n) or 0)

    def camera(cam=c, gs=g, rs=s, bufs=b, grad2d=fake, depth_mode=0, scratch=fake, out=fake):
        ref = lambda x: None if x is None else ctypes.byref(x)
        return L.gsr_backward_camera(ref(cam), ref(gs), ref(rs), ref(bufs), grad2d, depth_mode, scratch, out, None)

    def posed(cam=c, gs=g, rs=s, bufs=b, dpix=fake, aux=None, al=alloc, grads=gr, out=fake):
        ref = lambda x: None if x is None else ctypes.byref(x)
        return L.gsr_backward_posed(ref(cam), ref(gs), ref(rs), ref(bufs), dpix, ref(aux), al, None, ref(grads), out,
                                    None)

    def check(rc, word, code=None):
        assert rc < 0 and (code is None or rc == code), rc
        assert word in native.last_error(), native.last_error()

    # null pointers
    for kw in (dict(cam=None), dict(gs=None), dict(rs=None)):
        check(camera(**kw), "null")
        check(posed(**kw), "null")
    for kw in (dict(bufs=None), dict(grad2d=None), dict(scratch=None), dict(out=None)):
        check(camera(**kw), "null")
    for kw in (dict(bufs=None), dict(dpix=None), dict(out=None), dict(al=ctypes.cast(None, native.ALLOC_FN))):
        check(posed(**kw), "null")
    check(posed(grads=None), "missing gradient outputs")
    # misaligned output
    check(camera(out=ctypes.c_void_p((1 << 20) + 4)), "aligned")
    check(posed(out=ctypes.c_void_p((1 << 20) + 4)), "aligned")
    # bad depth_mode
    for m in (-1, 3, 7):
        check(camera(depth_mode=m), "depth_mode")
    # a tile band
    band = native.Settings()
    band.tile_y0, band.tile_y1 = 1, 2
    check(camera(rs=band), "full images only")
    check(posed(rs=band), "full images only")
    # a layout word without the tag, and one that disagrees with the buffers
    for layout, word in ((0, "not a forward's"), (b.layout & ~1, "disagrees")):
        bad = native.Buffers()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(b), ctypes.sizeof(b))
        bad.layout = layout
        check(camera(bufs=bad), word, err_layout)
        check(posed(bufs=bad), word, err_layout)
    # the anti-alias flag against the layout bit, both ways
    aa = native.Settings()
    aa.tile_y1, aa.flags = 2**31 - 1, native.GSR_FLAG_ANTIALIAS
    check(camera(rs=aa), "GSR_FLAG_ANTIALIAS", err_layout)
    check(posed(rs=aa), "GSR_FLAG_ANTIALIAS", err_layout)
    baa = native.Buffers()
    ctypes.memmove(ctypes.byref(baa), ctypes.byref(b), ctypes.sizeof(b))
    baa.layout |= native.GSR_LAYOUT_ANTIALIAS
    check(camera(bufs=baa), "GSR_FLAG_ANTIALIAS", err_layout)
    check(posed(bufs=baa), "GSR_FLAG_ANTIALIAS", err_layout)
    # the aux form needs gsr_forward_aux's buffers
    check(posed(aux=native.AuxGrads()), "GSR_LAYOUT_AUX", err_layout)
    # buffers of another Gaussian count
    other = native.Buffers()
    ctypes.memmove(ctypes.byref(other), ctypes.byref(b), ctypes.sizeof(b))
    other.n_local = 6
    check(camera(bufs=other), "do not match")
    check(posed(bufs=other), "do not match")
    assert calls == [], "nothing may be allocated before the checks"


# ---------------------------------------------------------------- pose module
def test_delta_matrix_closed_forms():
    pose = pkg("pose")
    D0 = pose.delta_matrix(torch.zeros(6, dtype=torch.float64))
    assert torch.equal(D0, torch.eye(4, dtype=torch.float64))
    rng = np.random.default_rng(3)
    for scale in (1e-9, 1e-5, 1e-2, 0.3, 2.5):
        d = torch.tensor(np.concatenate([scale * rng.standard_normal(3), rng.standard_normal(3)]))
        D = pose.delta_matrix(d)
        R = D[:3, :3]
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-14, rtol=0)
        assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-14
        assert torch.equal(D[3, :3], d[3:]) and torch.equal(D[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
        # Exp(omega) fixes its axis and turns by |omega|: trace = 1 + 2 cos t
        w = d[:3]
        assert torch.allclose(R.T @ w, w, atol=1e-14 * max(1.0, float(w.norm())), rtol=0)
        assert abs(float(torch.trace(R)) - (1.0 + 2.0 * math.cos(float(w.norm())))) < 1e-14
    # a quarter turn about z, in the row-vector convention: D[:3, :3] = Exp(omega)^T
    Dz = pose.delta_matrix(torch.tensor([0.0, 0.0, math.pi / 2, 0.0, 0.0, 0.0], dtype=torch.float64))
    want = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)  # Exp
    assert torch.allclose(Dz[:3, :3], want.T, atol=1e-15, rtol=0)


def test_series_and_rodrigues_agree_at_the_switch():
    pose = pkg("pose")
    rng = np.random.default_rng(4)
    for _ in range(8):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        for t in (pose.SERIES_BELOW * (1 - 1e-9), pose.SERIES_BELOW, pose.SERIES_BELOW * (1 + 1e-9)):
            w = torch.tensor(axis * t)
            a, b = pose.so3_exp(w, series=True), pose.so3_exp(w, series=False)
            # the series' first dropped terms are t^6 / 5040 and t^6 / 40320 of K, K^2: ~1e-22 here
            assert float((a - b).abs().max()) < 1e-15
    # the automatic choice takes each branch on its side
    w = torch.tensor([pose.SERIES_BELOW * 0.5, 0.0, 0.0], dtype=torch.float64)
    assert torch.equal(pose.so3_exp(w), pose.so3_exp(w, series=True))
    w = torch.tensor([pose.SERIES_BELOW * 2.0, 0.0, 0.0], dtype=torch.float64)
    assert torch.equal(pose.so3_exp(w), pose.so3_exp(w, series=False))


def test_compose_zero_reproduces_the_camera_bit_for_bit():
    pose = pkg("pose")
    cams = [_camera()] + pkg("train_loop").orbit_cameras(5, 96, 64, seed=2)
    for cam in cams:
        got = pose.compose(cam, torch.zeros(6, dtype=torch.float64))
        for f in ("viewmatrix", "projmatrix", "campos"):
            a, b = np.asarray(getattr(got, f)), np.asarray(getattr(cam, f))
            assert a.dtype == np.float32 and a.shape == b.shape
            assert a.tobytes() == b.tobytes(), f
        assert (got.width, got.height, got.tanfovx, got.tanfovy, got.znear, got.zfar) == \
            (cam.width, cam.height, cam.tanfovx, cam.tanfovy, cam.znear, cam.zfar)
        assert pose.pose_error(cam, got) == (0.0, 0.0)


def test_compose_is_the_camera_of_the_moved_pose():
    """compose(cam, delta) is, up to f32 rounding, the camera make_camera builds from the moved pose:
    full_proj = world_view' @ proj and campos = inv(world_view')[3, :3]."""
    pose, graphics = pkg("pose"), pkg("graphics")
    cam = _camera()
    d = torch.tensor([0.02, -0.035, 0.015, 0.08, -0.05, 0.11], dtype=torch.float64)
    got = pose.compose(cam, d)
    wv = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4) @ pose.delta_matrix(d).numpy()
    proj = graphics.get_projection_matrix(cam.znear, cam.zfar, 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)).T
    np.testing.assert_allclose(np.asarray(got.viewmatrix, np.float64).reshape(4, 4), wv, rtol=0, atol=2e-7)
    np.testing.assert_allclose(np.asarray(got.projmatrix, np.float64).reshape(4, 4), wv @ proj, rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.asarray(got.campos, np.float64), np.linalg.inv(wv)[3, :3], rtol=0, atol=1e-6)
    ang, dist = pose.pose_error(cam, got)
    assert abs(ang - float(d[:3].norm())) < 1e-6
    # the centre moves by -R^T tau (rotated into the world): |centre' - centre| from the two view matrices
    c0, c1 = np.linalg.inv(np.asarray(cam.viewmatrix, np.float64).reshape(4, 4))[3, :3], np.linalg.inv(wv)[3, :3]
    assert abs(dist - np.linalg.norm(c1 - c0)) < 1e-6


def test_chain_against_central_differences():
    pose = pkg("pose")
    cam = _camera()
    rng = np.random.default_rng(5)
    for d0 in (np.zeros(6), np.array([0.03, -0.02, 0.05, 0.1, -0.2, 0.05]), np.array([1e-5, 0, 0, 0, 0.3, 0]),
               np.array([0.9, -1.2, 0.4, -0.6, 0.2, 0.7])):
        w = rng.standard_normal(36)
        w[35] = 0.0

        def f(d):
            v, p, c = pose._fields(cam, torch.tensor(d, dtype=torch.float64))
            return float((v * torch.tensor(w[0:16])).sum() + (p * torch.tensor(w[16:32])).sum() +
                         (c * torch.tensor(w[32:35])).sum())

        got = pose.chain(cam, torch.tensor(d0), torch.tensor(w, dtype=torch.float32).double()).numpy()
        h = 1e-5
        ref = np.array([(f(d0 + h * e) - f(d0 - h * e)) / (2 * h) for e in np.eye(6)])
        # central differences: truncation h^2 f''' / 6 ~ 1e-10 |f|, rounding eps |f| / h ~ 1e-10 |f|; |f| ~ 30
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-7 * (1.0 + np.abs(ref).max()))
        assert got.dtype == np.float64 and got.shape == (6,)


# ---------------------------------------------------------------- trainer options
def test_optimization_params_and_schedule():
    T, general = pkg("trainer"), pkg("general")
    o = T.OptimizationParams()
    assert o.train_poses is False
    assert (o.pose_lr_init, o.pose_lr_final) == (1e-4, 1e-6)
    assert (o.pose_lr_delay_steps, o.pose_lr_delay_mult) == (0, 0.0)
    f = general.get_expon_lr_func(o.pose_lr_init, o.pose_lr_final, lr_delay_steps=o.pose_lr_delay_steps,
                                  lr_delay_mult=o.pose_lr_delay_mult, max_steps=o.iterations)
    assert math.isclose(f(0), 1e-4, rel_tol=1e-12) and math.isclose(f(o.iterations), 1e-6, rel_tol=1e-12)


def test_pose_adam_row_matches_torch_adam():
    """The host-side per-row Adam is torch.optim.Adam's arithmetic with the row's own step count, the
    translation step scaled by spatial_lr_scale."""
    T = pkg("trainer")
    rng = np.random.default_rng(6)
    st = T.PoseState(3)
    ref = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=1.0, betas=(0.9, 0.999), eps=1e-8)
    lr, scale = 3e-3, 1.0
    for _ in range(5):
        g = rng.standard_normal(6)
        st.adam_row(1, g, lr, scale)
        ref.grad = torch.tensor(g)
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
    np.testing.assert_allclose(st.delta[1], ref.detach().numpy(), rtol=1e-12, atol=0)
    assert st.steps.tolist() == [0, 5, 0] and not st.delta[0].any() and not st.delta[2].any()
    st2 = T.PoseState(1)
    st2.adam_row(0, np.ones(6), 1e-2, 4.0)
    np.testing.assert_allclose(st2.delta[0], -1e-2 * np.array([1, 1, 1, 4, 4, 4.0]), rtol=1e-6)


def test_write_scene_refuses_train_poses(tmp_path):
    L, T = pkg("train_loop"), pkg("trainer")
    scene = L.LoopScene(cams=[], gts=[], points=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.float32),
                        extent=1.0)
    with pytest.raises(ValueError, match="pose"):
        L.write_scene(str(tmp_path / "scene.bin"), scene, 10, opt=T.OptimizationParams(train_poses=True))


def test_pose_state_round_trip(tmp_path):
    T, sio = pkg("trainer"), pkg("scene_io")
    st = T.PoseState(4)
    rng = np.random.default_rng(7)
    for i in range(7):
        st.adam_row(int(rng.integers(0, 4)), rng.standard_normal(6), 1e-3, 2.0)
    path = str(tmp_path / "pose.ckpt")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    params = {"xyz": z(2, 3), "f_dc": z(2, 1, 3), "f_rest": z(2, 3, 3), "opacity": z(2, 1), "scaling": z(2, 3),
              "rotation": z(2, 4)}
    state = {"active_sh_degree": 1, "spatial_lr_scale": 2.0, "params": params, "max_radii2D": z(2),
             "xyz_gradient_accum": z(2), "denom": z(2), "exp_avg": {k: v.clone() for k, v in params.items()},
             "exp_avg_sq": {k: v.clone() for k, v in params.items()}, "steps": {k: 0 for k in params}}
    sio.save_checkpoint(path, dict(state, poses=st.state_dict()))
    back = T.PoseState.from_state_dict(sio.load_checkpoint(path, "cpu")["poses"])
    plain = str(tmp_path / "plain.ckpt")
    sio.save_checkpoint(plain, state)
    assert sio.load_checkpoint(plain, "cpu")["poses"] is None  # a checkpoint without poses restores as before
    for name in ("delta", "exp_avg", "exp_avg_sq", "steps"):
        a, b = getattr(st, name), getattr(back, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def test_pose_options_are_validated():
    T = pkg("trainer")
    z = lambda *shape: np.zeros(shape, np.float32)
    make = lambda **kw: T.GaussianTrainer(z(2, 3), z(2, 1, 3), z(2, 3, 3), z(2, 1), z(2, 3), z(2, 4), 1,
                                          opt=T.OptimizationParams(**kw), device="cpu")
    for bad in (dict(pose_lr_init=-1e-4), dict(pose_lr_final=-1.0), dict(pose_lr_init=float("nan")),
                dict(pose_lr_final=float("inf")), dict(pose_lr_delay_mult=-0.5), dict(pose_lr_delay_steps=-1),
                dict(pose_lr_init=0.0), dict(pose_lr_final=0.0)):
        with pytest.raises(ValueError, match="pose_lr"):
            make(**bad)
    make(pose_lr_init=0.0, pose_lr_final=0.0)  # frozen poses
    tr = make(train_poses=True)
    assert tr.pose_lr == 1e-4
    tr.update_learning_rate(tr.opt.iterations)
    assert math.isclose(tr.pose_lr, 1e-6, rel_tol=1e-12)


def test_step_refuses_bad_pose_arguments_before_any_device_call():
    T = pkg("trainer")
    z = lambda *shape: np.zeros(shape, np.float32)
    tr = T.GaussianTrainer(z(2, 3), z(2, 1, 3), z(2, 3, 3), z(2, 1), z(2, 3), z(2, 4), 1,
                           opt=T.OptimizationParams(train_poses=True), device="cpu")
    cam, gt = _camera(), torch.zeros(3, 64, 96)
    with pytest.raises(ValueError, match="setup_poses"):
        tr.step(1, cam, gt, view_index=0)
    with pytest.raises(ValueError, match="positive"):
        tr.setup_poses(0)
    tr.setup_poses(3)
    assert tr.poses.delta.shape == (3, 6) and tr.poses.delta.dtype == np.float64 and not tr.poses.delta.any()
    with pytest.raises(ValueError, match="view_index"):
        tr.step(1, cam, gt)
    for v in (-1, 3, 17):
        with pytest.raises(ValueError, match="outside the 3 pose rows"):
            tr.step(1, cam, gt, view_index=v)
    with pytest.raises(ValueError, match="one camera per pose row"):
        tr.refined_cameras([cam])
    got = tr.refined_cameras([cam, cam, cam])
    assert all(np.asarray(c.viewmatrix).tobytes() == np.asarray(cam.viewmatrix).tobytes() for c in got)
    assert tr.steps == {k: 0 for k in T.GROUPS} and not tr._pose_pending  # nothing ran
