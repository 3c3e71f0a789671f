"""Depth-supervised training on the GPU: the fused depth-loss kernel (gsr_depth_loss) through the
C ABI and the libtorch autograd Function, and GaussianTrainer.step(gt_depth=...) on top of it.

Bars (the project's for the photometric loss, tests/test_gpu_train.py):
  * stats[0], stats[1]: relative 1e-5 against an fp64 restatement; stats[2] (pixel count) exact;
  * dL/ddepth, dL/dalpha: relative L2 1e-5, element-wise 1e-5 of the largest element, and exact
    zeros at masked, zero-residual and low-alpha pixels;
  * two calls, the unaligned scalar path and the autograd Function: equal bits;
  * one supervised step vs the CPU composite: exp_avg (= 0.1 x the raw gradient after step 1)
    within relative L2 1e-4, and the depth term moves exp_avg["xyz"] by more than 100x that bar.

Inputs keep |pred - target| either exactly 0 or >= 1e-3 (asserted on the fp64 side), so a sign is
never a rounding matter.
"""
import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

import train_oracle as T
from test_native_aux import aux_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA_MIN = 0.5
f32 = np.float32


@pytest.fixture(scope="module")
def K():
    return pkg("trainer").TrainKernels(DEV)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


# ---------------------------------------------------------------------------------------------
# 1. the kernel against an fp64 restatement
# ---------------------------------------------------------------------------------------------
def make_case(shape, normalized, masked, seed):
    """depth / alpha / target / mask planes with every special pixel class the kernel treats:
    exact zero residuals (target copied from depth, alpha == 1), alpha just below / at / just above
    ALPHA_MIN, mask zeros and fractional mask values."""
    H, W = shape
    n = H * W
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)
    k = n // 8
    below, at, above, zero = idx[:k], idx[k:2 * k], idx[2 * k:3 * k], idx[3 * k:4 * k]
    depth = rng.uniform(0.1, 3.0, n).astype(f32)
    alpha = None
    if normalized:
        alpha = rng.uniform(0.05, 1.0, n).astype(f32)
        alpha[below] = np.nextafter(f32(ALPHA_MIN), f32(0.0))
        alpha[at] = f32(ALPHA_MIN)
        alpha[above] = np.nextafter(f32(ALPHA_MIN), f32(1.0))
        alpha[zero] = 1.0
        depth = (depth * alpha).astype(f32)  # a blended depth: about alpha x the surface's
    pred = depth.astype(np.float64) / (alpha.astype(np.float64) if normalized else 1.0)
    delta = rng.uniform(2e-3, 0.5, n) * rng.choice([-1.0, 1.0], n)
    target = (pred + delta).astype(f32)
    target[zero] = depth[zero]
    mask = None
    if masked:
        mask = rng.uniform(0.1, 1.0, n).astype(f32)
        mask[rng.random(n) < 0.3] = 0.0
        mask[rng.random(n) < 0.2] = 1.0
    r = lambda a: None if a is None else a.reshape(H, W)
    return dict(depth=r(depth), alpha=r(alpha), target=r(target), mask=r(mask), zero=zero,
                low=below if normalized else idx[:0])


def reference(c, weight, normalized):
    """fp64 torch restatement: weight * mean |(pred - target) * m|, gradients by autograd."""
    dt = torch.float64
    d = torch.tensor(c["depth"], dtype=dt, requires_grad=True)
    t = torch.tensor(c["target"], dtype=dt)
    m = torch.ones_like(t) if c["mask"] is None else torch.tensor(c["mask"], dtype=dt)
    a = None
    if normalized:
        a = torch.tensor(c["alpha"], dtype=dt, requires_grad=True)
        ok = a >= ALPHA_MIN
        pred = d / torch.where(ok, a, torch.ones_like(a))
        m = m * ok
    else:
        pred = d
    res = (pred - t).detach().abs()[m != 0]
    assert bool(((res == 0) | (res >= 1e-3)).all()), "a residual inside (0, 1e-3): the sign would be a rounding matter"
    l1 = ((pred - t) * m).abs().mean()
    (weight * l1).backward()
    l1 = float(l1.detach())
    return dict(stats=(weight * l1, l1, int((m != 0).sum())), dd=d.grad.numpy(),
                da=a.grad.numpy() if normalized else None, live=(m != 0).numpy())


def check_case(K, c, weight, normalized, planes=None):
    ref = reference(c, weight, normalized)
    p = planes or {k: (None if c[k] is None else _t(c[k])) for k in ("depth", "alpha", "target", "mask")}
    stats, dd, da = K.depth_loss(p["depth"], p["target"], mask=p["mask"], alpha=p["alpha"] if normalized else None,
                                 weight=weight, normalized=normalized, alpha_min=ALPHA_MIN)
    st = stats.cpu().numpy().astype(np.float64)
    print("stats", st, ref["stats"])
    for got, want in zip(st[:2], ref["stats"][:2]):
        assert abs(got - want) <= 1e-5 * abs(want), (st, ref["stats"])
    assert st[2] == ref["stats"][2]
    assert (da is None) == (not normalized)
    dead = ~ref["live"].reshape(-1)
    dead[c["zero"]] = True
    dead[c["low"]] = True
    for name, got, want in (("dd", dd, ref["dd"]), ("da", da, ref["da"])):
        if got is None:
            continue
        g = got.cpu().numpy()
        print(name, "rel_l2", rel_l2(g, want), "max err / max", np.max(np.abs(g - want)) / max(np.max(np.abs(want)), 1e-300))
        assert rel_l2(g, want) <= 1e-5, name
        assert np.max(np.abs(g - want)) <= 1e-5 * np.max(np.abs(want)) + 1e-30, name
        assert not g.reshape(-1)[dead].any(), name  # exact zeros
        assert not want.reshape(-1)[dead].any()
    return stats, dd, da


SHAPES = [(1, 1), (1, 3), (16, 16), (70, 101), (33, 200)]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_fp64(K, shape, normalized, masked):
    """1x1, 1x3 (tail only), 16x16 (one full block row), 70x101 (n % 4 == 2, 7 chunks), 33x200."""
    c = make_case(shape, normalized, masked, seed=shape[0] * 1000 + shape[1] + 2 * normalized + masked)
    if shape[0] * shape[1] >= 64:
        assert len(c["zero"]) and (not normalized or len(c["low"]))
    check_case(K, c, 0.37, normalized)


@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
def test_kernel_multi_chunk_blocks(K, normalized):
    """The grid is min(ceil(n / 1024), 2048) blocks of 256 threads x 4 pixels, block b taking chunks
    b, b + 2048, ...: the smallest image in which a block handles more than one chunk has
    2048 * 1024 + 1 = 2 097 153 pixels (here 1 x 2097153, so the last chunk is a 1-pixel tail too);
    the finalize then sums 2048 > 256 partials."""
    c = make_case((1, 2048 * 1024 + 1), normalized, True, seed=11 + normalized)
    check_case(K, c, 1.0, normalized)


@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
def test_kernel_unaligned_planes(K, normalized):
    """Planes sliced at a 1-element offset (4-byte aligned only) take the scalar path: within the
    bars, and the same bits as the float4 path (same pixels per thread, same sums)."""
    shape = (70, 101)
    n = shape[0] * shape[1]
    c = make_case(shape, normalized, True, seed=5 + normalized)
    aligned = check_case(K, c, 0.8, normalized)
    off = {}
    for k in ("depth", "alpha", "target", "mask"):
        if c[k] is None:
            off[k] = None
            continue
        buf = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
        buf[1:] = _t(c[k]).reshape(-1)
        off[k] = buf[1:].view(shape)
        assert off[k].data_ptr() % 16 == 4 and off[k].is_contiguous()
    shifted = check_case(K, c, 0.8, normalized, planes=off)
    for a, b in zip(aligned, shifted):
        assert (a is None and b is None) or torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# 2. determinism, and the autograd Function against the C ABI
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
def test_deterministic_and_autograd_function_equal_bits(K, normalized):
    R, native = pkg("rasterizer"), pkg("native")
    ext = native.load_torch_ext()
    c = make_case((203, 301), normalized, True, seed=21 + normalized)
    p = {k: (None if c[k] is None else _t(c[k])) for k in ("depth", "alpha", "target", "mask")}
    kw = dict(mask=p["mask"], alpha=p["alpha"] if normalized else None, weight=0.6, normalized=normalized,
              alpha_min=ALPHA_MIN)
    s1, dd1, da1 = K.depth_loss(p["depth"], p["target"], **kw)
    s2, dd2, da2 = K.depth_loss(p["depth"], p["target"], **kw)
    assert torch.equal(s1, s2) and torch.equal(dd1, dd2)
    assert (not normalized) or torch.equal(da1, da2)
    d = p["depth"].clone().requires_grad_(True)
    a = p["alpha"].clone().requires_grad_(True) if normalized else None
    mode = native.DEPTH_NORMALIZED if normalized else native.DEPTH_RAW
    loss, stats = ext.depth_loss(d, a, p["target"], p["mask"], 0.6, mode, ALPHA_MIN)
    assert loss.shape == () and loss.is_cuda and torch.equal(stats, s1) and torch.equal(loss, s1[0])
    grads = torch.autograd.grad(loss, [d, a] if normalized else [d])
    assert torch.equal(grads[0], dd1)
    assert (not normalized) or torch.equal(grads[1], da1)
    # the rasterizer.py wrapper, and an incoming gradient other than 1 (scaled on the device)
    d2 = p["depth"].clone().requires_grad_(True)
    l2, st2 = R.depth_loss(d2, p["target"], mask=p["mask"], alpha=a.detach() if normalized else None, weight=0.6,
                           normalized=normalized, alpha_min=ALPHA_MIN, return_stats=True)
    assert torch.equal(st2, s1)
    (3.0 * l2).backward()
    assert torch.equal(d2.grad, dd1 * 3.0)


# ---------------------------------------------------------------------------------------------
# 3 - 5. the trainer's supervised step
# ---------------------------------------------------------------------------------------------
def np_depth_loss(depth, alpha, target, mask, weight, normalized):
    """The depth loss and its gradients in numpy fp64 (include/gsr/gsr_train.h semantics)."""
    d, t, m = (np.asarray(x, np.float64) for x in (depth, target, mask))
    a = np.ones_like(d)
    if normalized:
        ok = np.asarray(alpha, f32) >= f32(ALPHA_MIN)
        a = np.where(ok, np.asarray(alpha, np.float64), 1.0)
        m = m * ok
    e = (d / a - t) * m
    gp = weight / d.size * m * np.sign(e)
    dd = gp / a
    da = -gp * d / a ** 2 if normalized else None
    return float(np.abs(e).mean()), dd, da


@pytest.fixture(scope="module")
def step_scene(oracle):
    """3000 Gaussians / 160x120 / SH3 (test_training_step_matches_cpu_composite's scene): the oracle's
    colour, inverse depth and alpha, computed once and shared."""
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(160, 120)
    s = sc.make_scene(cam, 3000, max_sh_degree=3, seed=3)
    gt = np.random.default_rng(4).random((3, 120, 160)).astype(f32)
    sc_, q_, o_ = T.activate(s.raw_scales, s.raw_rotations, s.raw_opacities.reshape(-1, 1))
    inputs = dict(means3D=s.means3D, opacities=o_.reshape(-1), scales=sc_, rotations=q_, sh_dc=s.sh_dc,
                  sh_rest=s.sh_rest)
    fwd = aux_reference(oracle, cam, inputs, 3, np.zeros((3, 120, 160), f32), inverse=True)
    return dict(cam=cam, s=s, gt=gt, inputs=inputs, fwd=fwd)


def _trainer(s, **opt):
    Tr = pkg("trainer")
    tr = Tr.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                            s.raw_rotations, max_sh_degree=3, opt=Tr.OptimizationParams(**opt), device=DEV)
    tr.active_sh_degree = 3
    return tr


def _depth_target(fwd, normalized, seed):
    """A target at least 2 % of the largest prediction away from the oracle's prediction at every
    pixel (the GPU's prediction differs from the oracle's by rounding only, so every sign agrees),
    and a mask with zeros: 10 % at random, and in normalised mode every pixel whose alpha is within
    1e-3 of ALPHA_MIN (there a rounding difference could flip the alpha test)."""
    rng = np.random.default_rng(seed)
    depth, alpha = fwd["depth"].astype(np.float64), fwd["alpha"].astype(np.float64)
    ok = alpha >= ALPHA_MIN
    pred = np.where(ok, depth / np.where(ok, alpha, 1.0), 0.0) if normalized else depth
    scale = np.abs(pred).max()
    delta = rng.uniform(0.02, 0.2, pred.shape) * scale * rng.choice([-1.0, 1.0], pred.shape)
    mask = (rng.random(pred.shape) >= 0.1).astype(f32)
    if normalized:
        mask[np.abs(alpha - ALPHA_MIN) < 1e-3] = 0.0
    return (pred + delta).astype(f32), mask


@pytest.mark.parametrize("normalized", [False, True], ids=["raw_invdepth", "normalized"])
def test_supervised_step_matches_cpu_composite(oracle, step_scene, normalized):
    """One supervised iteration (activate -> gsr_forward_aux -> photometric loss -> gsr_depth_loss ->
    gsr_backward_aux -> statistics -> fused Adam) against the CPU composite: oracle forward,
    train_oracle.ssim_loss, the depth loss in numpy, aux_reference's gradients, raw_grads.  After
    step 1 exp_avg = (1 - beta1) x the raw gradient, which shows a mis-scaled depth term that
    Adam's first parameter move (lr sign(g)) would hide."""
    Tr = pkg("trainer")
    cam, s, gt, fwd = (step_scene[k] for k in ("cam", "s", "gt", "fwd"))
    target, mask = _depth_target(fwd, normalized, seed=6 + normalized)
    tr = _trainer(s, depth_normalized=normalized, depth_alpha_min=ALPHA_MIN)
    out = tr.step(1, cam, _t(gt), densify=False, gt_depth=_t(target), depth_mask=_t(mask))
    weight = tr.depth_weight_scheduler(1)
    assert 0.99 < weight < 1.0
    # CPU composite
    loss, _, _, dimg = T.ssim_loss(fwd["color"].astype(f32), gt, 0.2)
    l1d, dd, da = np_depth_loss(fwd["depth"], fwd["alpha"], target, mask, weight, normalized)
    st, dst = out["stats"].cpu().numpy(), out["depth_stats"].cpu().numpy()
    print("stats", st, loss, "depth_stats", dst, weight * l1d, l1d)
    assert abs(st[0] - loss) <= 1e-4 * abs(loss)
    assert abs(dst[1] - l1d) <= 1e-4 * l1d and abs(dst[0] - weight * l1d) <= 1e-4 * weight * l1d
    assert set(out) >= {"stats", "depth_stats", "depth", "alpha", "radii", "image"}
    ref = aux_reference(oracle, cam, step_scene["inputs"], 3, dimg, dd, da, inverse=True)
    g = ref["grads"]
    ds, dq, do = T.raw_grads(s.raw_scales, s.raw_rotations, s.raw_opacities.reshape(-1, 1), g["scales"],
                             g["rotations"], g["opacities"].reshape(-1, 1))
    graw = {"xyz": g["means3D"], "f_dc": g["sh_dc"], "f_rest": g["sh_rest"], "opacity": do, "scaling": ds,
            "rotation": dq}
    for k in Tr.GROUPS:
        m = tr.exp_avg[k].cpu().numpy()
        r = rel_l2(m, 0.1 * np.asarray(graw[k], np.float64).reshape(m.shape))
        print(k, "exp_avg rel_l2", r)
        assert r <= 1e-4, (k, r)
    # a dropped depth term fails: it moves the xyz moment by far more than the bar
    plain = _trainer(s)
    plain.step(1, cam, _t(gt), densify=False)
    moved = rel_l2(tr.exp_avg["xyz"].cpu().numpy(), plain.exp_avg["xyz"].cpu().numpy())
    print("depth term moves exp_avg[xyz] by", moved)
    assert moved > 100 * 1e-4


def test_unsupervised_paths_are_the_colour_only_step(step_scene):
    """No target, and a target at scheduled weight 0: the plain forward / backward, bit-identical
    parameters and moments, no depth keys."""
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    target, mask = _depth_target(step_scene["fwd"], False, seed=8)
    a, b = _trainer(s), _trainer(s, depth_l1_weight_init=0.0, depth_l1_weight_final=0.0)
    for it in (1, 2):
        oa = a.step(it, cam, _t(gt), densify=False)
        ob = b.step(it, cam, _t(gt), densify=False, gt_depth=_t(target), depth_mask=_t(mask))
        assert "depth_stats" not in oa and "depth_stats" not in ob
        assert set(oa) == set(ob) == {"stats", "radii", "state", "image", "num_points"}
        assert oa["state"].depth is None and ob["state"].depth is None
        assert torch.equal(oa["stats"], ob["stats"])
    for k in pkg("trainer").GROUPS:
        assert torch.equal(a.params[k], b.params[k]), k
        assert torch.equal(a.exp_avg[k], b.exp_avg[k]) and torch.equal(a.exp_avg_sq[k], b.exp_avg_sq[k]), k


def test_supervised_steps_render_under_the_bound(step_scene):
    """Three supervised steps: one exact sizing (the first render), then bounded renders without a
    host read of K, none of them overflowing."""
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    target, mask = _depth_target(step_scene["fwd"], False, seed=9)
    tr = _trainer(s)
    for it in (1, 2, 3):
        out = tr.step(it, cam, _t(gt), densify=False, gt_depth=_t(target), depth_mask=_t(mask))
        assert "depth_stats" in out
    torch.cuda.synchronize()
    tr.binning.poll()
    assert tr.binning.exact_reads == 1 and tr.binning.overflows == 0
    assert not tr.binning.pending  # both bounded renders were checked


# ---------------------------------------------------------------------------------------------
# 6 - 7. the loop's synthetic depth targets
# ---------------------------------------------------------------------------------------------
N_GT, LOOP_W, LOOP_H = 4000, 96, 64


@pytest.fixture(scope="module")
def depth_scene():
    L = pkg("train_loop")
    scene = L.synthetic_scene(N_GT, 500, 2, LOOP_W, LOOP_H, seed=0, device=DEV, gt_scale=0.05, with_depth=True)
    leaves = L.procedural_cloud(N_GT, 0, 0.25, 0.05)[:6]  # means, f_dc, f_rest, opacity, log scales, quaternions
    return scene, leaves


def _gt_trainer(scene, leaves, means=None, **opt):
    Tr = pkg("trainer")
    xyz, f_dc, f_rest, opac, log_s, q = leaves
    return Tr.GaussianTrainer(xyz if means is None else means, f_dc, f_rest, opac, log_s, q, max_sh_degree=1,
                              opt=Tr.OptimizationParams(**opt), spatial_lr_scale=scene.extent, device=DEV)


def test_self_target_has_zero_depth_loss(depth_scene):
    """A trainer holding the ground-truth leaves renders its own depth target: mean |e| is exactly
    0, every dL/ddepth is 0, and the stored target is forward_aux(inverse_depth=True).depth."""
    scene, leaves = depth_scene
    assert scene.depths is not None and len(scene.depths) == len(scene.cams) and scene.depth_masks is None
    plain = pkg("train_loop").synthetic_scene(N_GT, 500, 2, LOOP_W, LOOP_H, seed=0, device=DEV, gt_scale=0.05)
    assert plain.depths is None and all(torch.equal(a, b) for a, b in zip(plain.gts, scene.gts))
    tr = _gt_trainer(scene, leaves)
    out = tr.step(1, scene.cams[0], scene.gts[0], gt_depth=scene.depths[0])
    ds = out["depth_stats"].cpu().numpy()
    assert ds[1] == 0.0 and ds[0] == 0.0 and ds[2] == LOOP_W * LOOP_H
    assert not out["dL_ddepth"].any()
    assert torch.equal(out["depth"], scene.depths[0])
    assert float(scene.depths[0].max()) > 0.0  # and it is a depth image, not an empty one
    # an independent forward_aux of the activated ground truth
    k, rast = pkg("trainer").TrainKernels(DEV), pkg("rasterizer").CAbiRasterizer(DEV)
    xyz, f_dc, f_rest, opac, log_s, q = (_t(a) for a in leaves)
    sa, qa, oa = k.activate(log_s, q, opac)
    st = rast.forward_aux(scene.cams[1], xyz, oa.reshape(-1), scales=sa, rotations=qa, sh_dc=f_dc, sh_rest=f_rest,
                          sh_degree=1, inverse_depth=True)
    assert torch.equal(st.depth, scene.depths[1])
    with pytest.raises(ValueError, match="depth"):
        pkg("train_loop").write_scene("/dev/null", scene, 10)


def test_depth_supervision_descends(depth_scene):
    """The ground-truth cloud with every mean pushed 0.05 along the camera's view axis, 60
    supervised iterations of one view at depth weight 1, no densification: the last mean |e| is
    strictly below the first (the measured ratio is in DESIGN.md §9d)."""
    scene, leaves = depth_scene
    cam = scene.cams[0]
    V = np.asarray(cam.viewmatrix, np.float64).reshape(-1)
    axis = np.array([V[2], V[6], V[10]])
    axis /= np.linalg.norm(axis)
    means = (leaves[0].astype(np.float64) + 0.05 * axis[None, :]).astype(f32)
    tr = _gt_trainer(scene, leaves, means=means, depth_l1_weight_init=1.0, depth_l1_weight_final=1.0)
    log = []
    for it in range(1, 61):
        out = tr.step(it, cam, scene.gts[0], densify=False, gt_depth=scene.depths[0])
        if it in (1, 60):
            log.append(out["depth_stats"])
    first, last = (float(s[1]) for s in log)
    print("depth mean |e| first", first, "last", last, "ratio", last / first)
    assert first > 0.0 and last < first


def test_train_loop_passes_the_depth_targets(depth_scene):
    """train() over a scene with depth targets: every iteration is supervised and the depth loss is
    logged beside the photometric one; the same scene without them trains on colour only."""
    L, Tr = pkg("train_loop"), pkg("trainer")
    scene, _ = depth_scene
    res = L.train(scene, opt=Tr.OptimizationParams(iterations=4), max_sh_degree=1, log_every=2, device=DEV)
    assert [r[0] for r in res.depth_loss] == [r[0] for r in res.loss] == [1, 2, 4]
    for it, weighted, l1, pixels in res.depth_loss:
        w = res.trainer.depth_weight_scheduler(it)
        assert l1 > 0.0 and pixels == LOOP_W * LOOP_H and abs(weighted - w * l1) <= 1e-6 * w * l1
    assert res.binning_overflows == 0
    plain = L.LoopScene(cams=scene.cams, gts=scene.gts, points=scene.points, colors=scene.colors,
                        extent=scene.extent, n_gt=scene.n_gt)
    assert L.train(plain, opt=Tr.OptimizationParams(iterations=2), max_sh_degree=1, log_every=1,
                   device=DEV).depth_loss == []
