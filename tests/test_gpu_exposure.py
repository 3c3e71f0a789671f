"""Trained per-view exposure on the GPU: the gsr_exposure_forward / gsr_exposure_backward kernels
through the C ABI, the libtorch autograd Function and rasterizer.render(exposure=...), and
GaussianTrainer.step(view_index=...) with OptimizationParams.train_exposure on top of them.

The reference throughout is an fp64 torch restatement of upstream's expression
    matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
(clamped to [0, 1] with the flag), gradients by autograd.

Bars:
  * out: |got - ref| <= 1e-6 (sum_i |E_ij x_i| + |E_j3|) per element;
  * dL/dimg: relative L2 1e-5, element-wise 1e-5 of the largest element, exact zeros where the
    reference is zero;
  * every dL/dexposure entry: |got - ref| <= 1e-5 sum_p |term|, the absolute terms of the same sum
    taken from the fp64 reference.  The terms cancel, so a bar relative to the result would measure
    the cancellation; an f32 product plus a shuffle and LDS tree of about 16 roundings is about 1e-6
    of sum |term|, the bar is ten times that (the 1e-5 of the loss kernels);
  * the float4 and the scalar path, two calls, and every layer above the C ABI: equal bits.

Generated inputs keep every y_j at least 1e-3 away from 0 and 1 (asserted in fp64), so the clamp
mask is never a rounding matter; the identity case puts y exactly ON the bounds instead, where the
gradient must pass.  No pixel is excluded from any comparison.
"""
import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

import train_oracle as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
E_GENERAL = np.array([[0.90, 0.25, -0.30, 0.12],
                      [-0.35, 1.10, 0.20, -0.15],
                      [0.30, -0.25, 0.80, 0.20]], f32)  # off-diagonal terms, mixed signs, non-zero bias
E_TRUE = np.array([[0.85, 0.04, -0.03, 0.03],
                   [-0.05, 1.08, 0.02, -0.02],
                   [0.03, -0.04, 0.92, 0.04]], f32)     # gains 0.8 .. 1.1, cross terms <= 0.05, biases <= 0.04


@pytest.fixture(scope="module")
def K():
    return pkg("trainer").TrainKernels(DEV)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


# ---------------------------------------------------------------------------------------------
# the fp64 restatement
# ---------------------------------------------------------------------------------------------
def upstream_exposure(img, E, clamp):
    """Upstream's expression (gaussian_renderer/__init__.py, use_trained_exp) on torch tensors."""
    y = torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
    return torch.clamp(y, 0.0, 1.0) if clamp else y


def reference(x, E, g, clamp):
    """fp64: out, dL/dimg and dL/dexposure for the upstream gradient g, by autograd; plus the bars'
    scales -- out_scale = sum_i |E_ij x_i| + |E_j3| per element and abs_terms (3, 4) = the sum of the
    absolute terms of every dL/dexposure entry."""
    dt = torch.float64
    xt = torch.tensor(np.asarray(x), dtype=dt, requires_grad=True)
    Et = torch.tensor(np.asarray(E), dtype=dt, requires_grad=True)
    gt = torch.tensor(np.asarray(g), dtype=dt)
    y = upstream_exposure(xt, Et, False).detach()
    out = upstream_exposure(xt, Et, clamp)
    (out * gt).sum().backward()
    Ed, xd = Et.detach(), xt.detach()
    out_scale = torch.einsum("ij,ihw->jhw", Ed[:, :3].abs(), xd.abs()) + Ed[:, 3].abs()[:, None, None]
    live = ((y >= 0) & (y <= 1)) if clamp else torch.ones_like(y, dtype=torch.bool)
    ga = gt.abs() * live
    abs_terms = torch.zeros(3, 4, dtype=dt)
    abs_terms[:, :3] = torch.einsum("ihw,jhw->ij", xd.abs(), ga)
    abs_terms[:, 3] = ga.sum(dim=(1, 2))
    return dict(y=y.numpy(), out=out.detach().numpy(), dimg=xt.grad.numpy(), dE=Et.grad.numpy(),
                out_scale=out_scale.numpy(), abs_terms=abs_terms.numpy())


def make_case(shape, seed, E=E_GENERAL):
    """x in [-0.25, 1.25] and a normal upstream gradient; pixels with a y_j within 1e-3 of 0 or 1
    are resampled until none is left."""
    H, W = shape
    n = H * W
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, (3, n)).astype(f32)
    E64 = np.asarray(E, np.float64)
    for _ in range(100):
        y = E64[:, :3].T @ x.astype(np.float64) + E64[:, 3:4]
        near = ((np.abs(y) < 1e-3) | (np.abs(y - 1.0) < 1e-3)).any(axis=0)
        if not near.any():
            break
        x[:, near] = rng.uniform(-0.25, 1.25, (3, int(near.sum()))).astype(f32)
    g = rng.standard_normal((3, n)).astype(f32)
    return dict(x=x.reshape(3, H, W), g=g.reshape(3, H, W), E=np.asarray(E, f32))


def assert_clear_of_the_bounds(ref, need_tails):
    y = ref["y"]
    assert not ((np.abs(y) < 1e-3) | (np.abs(y - 1.0) < 1e-3)).any(), "a y_j within 1e-3 of a clamp bound"
    if need_tails:
        assert (y < 0).mean() >= 0.05 and (y > 1).mean() >= 0.05, ((y < 0).mean(), (y > 1).mean())


def check_against(ref, out, dimg, dE, what=""):
    """The three bars; prints the measured ratios (1.0 = at the bar)."""
    o, d, e = (np.asarray(t.detach().cpu().numpy(), np.float64) for t in (out, dimg, dE))
    r_out = float(np.max(np.abs(o - ref["out"]) / (1e-6 * ref["out_scale"] + 1e-300)))
    dmax = float(np.max(np.abs(ref["dimg"])))
    r_l2 = rel_l2(d, ref["dimg"]) / 1e-5 if dmax > 0 else 0.0
    r_max = float(np.max(np.abs(d - ref["dimg"]))) / (1e-5 * dmax) if dmax > 0 else 0.0
    err_e = np.abs(e - ref["dE"])
    r_e = float(np.max(np.where(ref["abs_terms"] > 0, err_e / (1e-5 * ref["abs_terms"] + 1e-300), 0.0)))
    print(f"{what} error / bar: out {r_out:.3g}  dimg rel_l2 {r_l2:.3g}  dimg max {r_max:.3g}  dexposure {r_e:.3g}")
    assert (np.abs(o - ref["out"]) <= 1e-6 * ref["out_scale"]).all(), r_out
    if dmax > 0:
        assert rel_l2(d, ref["dimg"]) <= 1e-5, r_l2
    assert np.max(np.abs(d - ref["dimg"])) <= 1e-5 * dmax, r_max
    assert not d[ref["dimg"] == 0].any()  # exact zeros
    assert (err_e <= 1e-5 * ref["abs_terms"]).all(), (r_e, e, ref["dE"])


def run_kernels(K, c, clamp, tensors=None):
    x, g, E = tensors or (_t(c["x"]), _t(c["g"]), _t(c["E"]))
    out = K.exposure_forward(x, E, clamp=clamp)
    dimg, dE = K.exposure_backward(x, E, g, clamp=clamp)
    assert out.shape == x.shape and dimg.shape == x.shape and dE.shape == (3, 4)
    return out, dimg, dE


# ---------------------------------------------------------------------------------------------
# 1. the kernels against fp64
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 3), (16, 16), (70, 101), (33, 200)]


@pytest.mark.parametrize("clamp", [False, True], ids=["affine", "clamp"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_fp64(K, shape, clamp):
    """1x1, 1x3 (tail only), 16x16 (float4 groups only), 70x101 (n % 4 == 2: unaligned planes 1 and 2,
    so the scalar path, 7 chunks), 33x200 (float4 groups, 7 chunks with a partial last one)."""
    c = make_case(shape, seed=shape[0] * 1000 + shape[1])
    ref = reference(c["x"], c["E"], c["g"], clamp)
    assert_clear_of_the_bounds(ref, need_tails=shape[0] * shape[1] >= 64)
    check_against(ref, *run_kernels(K, c, clamp), what=f"{shape} clamp={clamp}")


@pytest.mark.parametrize("shape", [(1, 3), (16, 16), (33, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_clamp_bounds_are_inclusive(K, shape):
    """E = eye(3, 4) and x in {0, 0.25, 1}: y is exactly 0, 0.25 or 1, the output is x and the
    gradient passes at every pixel (torch.clamp's backward: zero only strictly outside)."""
    rng = np.random.default_rng(7)
    x = rng.choice(np.array([0.0, 0.25, 1.0], f32), (3,) + shape)
    g = rng.standard_normal((3,) + shape).astype(f32)
    c = dict(x=x, g=g, E=np.eye(3, 4, dtype=f32))
    ref = reference(x, c["E"], g, True)
    assert np.isin(ref["y"], [0.0, 0.25, 1.0]).all() and (ref["y"] == 0).any() and (ref["y"] == 1).any()
    np.testing.assert_array_equal(ref["dimg"], g.astype(np.float64))  # the reference passes it too
    out, dimg, dE = run_kernels(K, c, True)
    check_against(ref, out, dimg, dE, what=f"{shape} identity")
    assert torch.equal(out, _t(x)) and torch.equal(dimg, _t(g))


# ---------------------------------------------------------------------------------------------
# 2. blocks with more than one chunk
# ---------------------------------------------------------------------------------------------
def test_kernel_multi_chunk_blocks(K):
    """The grid is the depth loss's: min(ceil(n / 1024), 2048) blocks of 256 threads x 4 pixels, block
    b taking chunks b, b + 2048, ...  The smallest image in which a block takes a second chunk has
    2048 * 1024 + 1 = 2 097 153 pixels (here 1 x 2097153: that chunk is a 1-pixel tail, and the odd
    plane size puts planes 1 and 2 off 16 bytes); the finalize then sums 2048 > 256 partials."""
    c = make_case((1, 2048 * 1024 + 1), seed=11)
    ref = reference(c["x"], c["E"], c["g"], True)
    assert_clear_of_the_bounds(ref, need_tails=True)
    check_against(ref, *run_kernels(K, c, True), what="multi-chunk")


def test_kernel_multi_chunk_float4(K):
    """The same geometry with n % 4 == 0 (2 x 1048578 = 2048 * 1024 + 4 pixels), so that the second
    chunk runs on the float4 path."""
    c = make_case((2, 1024 * 1024 + 2), seed=12)
    ref = reference(c["x"], c["E"], c["g"], True)
    check_against(ref, *run_kernels(K, c, True), what="multi-chunk float4")


# ---------------------------------------------------------------------------------------------
# 3. unaligned planes, rows of larger tensors
# ---------------------------------------------------------------------------------------------
def test_kernel_unaligned_planes_and_rows(K):
    """Images at a one-float offset (4-byte aligned only) take the scalar path: within the bars and
    the bits of the float4 path.  exposure is row 1 of an (N, 3, 4) tensor and dL_dexposure lands in
    row 1 of a gradient tensor whose other rows stay as they were."""
    shape = (33, 200)  # n % 4 == 0: the aligned call moves float4
    n = shape[0] * shape[1]
    c = make_case(shape, seed=5)
    ref = reference(c["x"], c["E"], c["g"], True)
    assert_clear_of_the_bounds(ref, need_tails=True)
    assert _t(c["x"]).data_ptr() % 16 == 0
    aligned = run_kernels(K, c, True)
    check_against(ref, *aligned, what="aligned")
    off = []
    for a in (c["x"], c["g"]):
        buf = torch.zeros(3 * n + 1, dtype=torch.float32, device=DEV)
        buf[1:] = _t(a).reshape(-1)
        off.append(buf[1:].view((3,) + shape))
        assert off[-1].data_ptr() % 16 == 4 and off[-1].is_contiguous()
    rows = torch.full((3, 3, 4), 9.0, dtype=torch.float32, device=DEV)
    rows[1] = _t(c["E"])
    grad = torch.full((3, 3, 4), 7.0, dtype=torch.float32, device=DEV)
    out = K.exposure_forward(off[0], rows[1], clamp=True)
    dimg, dE = K.exposure_backward(off[0], rows[1], off[1], clamp=True, out=grad[1])
    check_against(ref, out, dimg, dE, what="offset")
    for a, b in zip(aligned, (out, dimg, dE)):
        assert torch.equal(a, b)
    assert dE.data_ptr() == grad[1].data_ptr() and torch.equal(grad[1], aligned[2])
    assert bool((grad[0] == 7.0).all()) and bool((grad[2] == 7.0).all())
    assert bool((rows[0] == 9.0).all()) and bool((rows[2] == 9.0).all()) and torch.equal(rows[1], _t(c["E"]))


# ---------------------------------------------------------------------------------------------
# 4. determinism, and the layers above the C ABI
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True], ids=["affine", "clamp"])
def test_deterministic_and_autograd_layers_equal_bits(K, clamp):
    R, native = pkg("rasterizer"), pkg("native")
    ext = native.load_torch_ext()
    c = make_case((203, 301), seed=21)
    x, g, E = _t(c["x"]), _t(c["g"]), _t(c["E"])
    a, b = run_kernels(K, c, clamp, (x, g, E)), run_kernels(K, c, clamp, (x, g, E))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for fn in (ext.apply_exposure, R.apply_exposure):
        xl, El = x.clone().requires_grad_(True), E.clone().requires_grad_(True)
        out = fn(xl, El, clamp)
        assert torch.equal(out, a[0])
        gx, gE = torch.autograd.grad(out, [xl, El], grad_outputs=g)
        assert torch.equal(gx, a[1]) and torch.equal(gE, a[2])
    # a scaled upstream gradient through autograd, against the fp64 reference
    xl, El = x.clone().requires_grad_(True), E.clone().requires_grad_(True)
    out = R.apply_exposure(xl, El, clamp)
    (3 * out.sum()).backward()
    ref = reference(c["x"], c["E"], np.full_like(c["g"], 3.0), clamp)
    check_against(ref, out, xl.grad, El.grad, what=f"3 * sum, clamp={clamp}")


def test_render_applies_the_exposure():
    gr, sc = pkg("graphics"), pkg("scene")
    R, M = pkg("rasterizer"), pkg("model")
    cam = gr.synthetic_camera(192, 144)
    s = sc.make_scene(cam, 3000, max_sh_degree=3, seed=3)
    model = M.GaussianModel.from_scene(s, "cuda")
    bg = torch.zeros(3, device="cuda")
    E = _t(E_TRUE)
    base = R.render(cam, model, R.PipelineParams(), bg)
    assert set(base) == {"render", "viewspace_points", "visibility_filter", "radii"}  # exactly today's keys
    for clamp in (False, True):
        out = R.render(cam, model, R.PipelineParams(), bg, exposure=E, clamp=clamp)
        assert set(out) == set(base) and torch.equal(out["radii"], base["radii"])
        assert torch.equal(out["render"], R.apply_exposure(base["render"], E, clamp))
        assert not torch.equal(out["render"], base["render"])
    aux = R.render(cam, model, R.PipelineParams(), bg, return_depth=True, exposure=E)
    assert torch.equal(aux["render"], R.apply_exposure(base["render"], E))
    # and the exposed render is differentiable down to the leaves and to the exposure
    El = E.clone().requires_grad_(True)
    out = R.render(cam, model, R.PipelineParams(), bg, exposure=El, clamp=True)
    out["render"].sum().backward()
    assert El.grad is not None and bool(El.grad.abs().sum() > 0)
    assert model._xyz.grad is not None and bool(model._xyz.grad.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------
# 5 - 7. the trainer's step
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_scene():
    """2000 Gaussians / 256 x 256 / SH3 and a random target."""
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(256, 256)
    s = sc.make_scene(cam, 2000, max_sh_degree=3, seed=3)
    gt = np.random.default_rng(4).random((3, 256, 256)).astype(f32)
    return dict(cam=cam, s=s, gt=gt)


def _trainer(s, **opt):
    Tr = pkg("trainer")
    tr = Tr.GaussianTrainer(s.means3D, s.sh_dc, s.sh_rest, s.raw_opacities.reshape(-1, 1), s.raw_scales,
                            s.raw_rotations, max_sh_degree=3, opt=Tr.OptimizationParams(**opt), device=DEV)
    tr.active_sh_degree = 3
    return tr


def test_identity_exposure_is_a_no_op(step_scene):
    """train_exposure with the initial eye(3, 4), no clamp and both exposure LRs 0 is the plain step
    bit for bit: x 1 + x' 0 + x'' 0 + 0 and g 1 + 0 + 0 are exact."""
    Tr = pkg("trainer")
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    a = _trainer(s)
    b = _trainer(s, train_exposure=True, exposure_clamp=False, exposure_lr_init=0.0, exposure_lr_final=0.0)
    b.setup_exposure(2)
    for it in (1, 2, 3):
        oa = a.step(it, cam, _t(gt), densify=False)
        ob = b.step(it, cam, _t(gt), densify=False, view_index=it % 2)
        assert torch.equal(oa["stats"], ob["stats"]), it
        assert torch.equal(oa["image"], ob["image"]) and torch.equal(ob["exposed"], ob["image"])
        assert set(ob) == set(oa) | {"exposed", "dL_dexposure"}
    for k in Tr.GROUPS:
        assert torch.equal(a.params[k], b.params[k]), k
        assert torch.equal(a.exp_avg[k], b.exp_avg[k]) and torch.equal(a.exp_avg_sq[k], b.exp_avg_sq[k]), k
    assert torch.equal(b.exposure, torch.eye(3, 4, device=DEV)[None].repeat(2, 1, 1))
    assert b.exposure_step == 3 and bool(b.exposure_exp_avg.abs().sum() > 0)  # the gradient did arrive


def test_step_needs_a_valid_view_index(step_scene):
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    tr = _trainer(s, train_exposure=True)
    with pytest.raises(ValueError, match="setup_exposure"):
        tr.step(1, cam, _t(gt), densify=False, view_index=0)
    tr.setup_exposure(2, names=["a", "b"])
    for bad in (None, -1, 2):
        with pytest.raises(ValueError, match="view_index"):
            tr.step(1, cam, _t(gt), densify=False, view_index=bad)
    with pytest.raises(ValueError):
        tr.setup_exposure(2, names=["a"])
    assert tr.steps["xyz"] == 0  # nothing ran


# a contrast stretch: on step_scene's render (values 0 .. 0.76) about 13 % of the y_j fall below 0 and
# 3 % above 1, so the clamp mask matters to every gradient the step test checks
E_START = np.array([[3.0, 0.20, -0.25, -0.5],
                    [-0.3, 3.20, 0.15, -0.6],
                    [0.2, -0.30, 2.80, -0.4]], f32)


def test_step_and_whole_tensor_adam_match_the_cpu_composite(oracle, step_scene):
    """Step 1 on view v = 1 of 3 from a non-identity exposure, clamp on, against the fp64 composite
    on the GPU's own render: upstream's expression, train_oracle.ssim_loss on the exposed image, the
    exposure backward by autograd; dL/dexposure at the kernel test's bar, exp_avg[v] = 0.1 x it,
    rows != v untouched, and the Gaussians' exp_avg["xyz"] against the oracle's backward of the
    composite's dL/dimage (relative L2 1e-4, test_supervised_step_matches_cpu_composite's).

    Step 2 on view u = 2: row v has no gradient and moves again on its decaying moments -- the whole
    (N, 3, 4) tensor is one Adam parameter, as upstream's exposure_optimizer has it.  Compared with
    torch.optim.Adam (CPU, fp64) fed the two recorded gradients: relative L2 1e-6, and every entry
    within 1e-6 of the largest one, 3.2 (the f32 half-ulp of the entries near 1 is 6e-8 and of those
    near 3 is 1.2e-7, per step: the bar is more than ten times that, and 1/2000 of row v's second
    move of about 7e-3)."""
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    v, u = 1, 2
    tr = _trainer(s, train_exposure=True, exposure_clamp=True)
    tr.setup_exposure(3)
    tr.exposure[v] = _t(E_START)
    start = tr.exposure.clone()
    out = tr.step(1, cam, _t(gt), densify=False, view_index=v)
    # ---- the fp64 composite
    dt = torch.float64
    x = torch.tensor(out["image"].cpu().numpy(), dtype=dt, requires_grad=True)
    E = torch.tensor(E_START, dtype=dt, requires_grad=True)
    exposed = upstream_exposure(x, E, True)
    loss, _, _, dexposed = T.ssim_loss(exposed.detach().numpy(), gt.astype(np.float64), 0.2, dtype=dt)
    ref = reference(x.detach().numpy(), E_START, dexposed, True)
    y = ref["y"]
    print("y below 0", (y < 0).mean(), "above 1", (y > 1).mean())
    assert (y < 0).mean() > 0.01 and (y > 1).mean() > 0.01
    st = out["stats"].cpu().numpy()
    assert abs(st[0] - loss) <= 1e-4 * abs(loss), (st, loss)
    assert (np.abs(out["exposed"].cpu().numpy() - ref["out"]) <= 1e-6 * ref["out_scale"]).all()
    dE = out["dL_dexposure"].cpu().numpy().astype(np.float64)
    ratio = np.abs(dE - ref["dE"]) / (1e-5 * ref["abs_terms"])
    print("dL_dexposure error / bar", ratio.max(), "\n", dE, "\n", ref["dE"])
    assert (np.abs(dE - ref["dE"]) <= 1e-5 * ref["abs_terms"]).all(), ratio
    assert np.abs(ref["dE"]).min() > 0
    # ---- the exposure's Adam state after step 1
    m = tr.exposure_exp_avg.cpu().numpy().astype(np.float64)
    assert (np.abs(m[v] - 0.1 * dE) <= 1e-6 * np.abs(0.1 * dE)).all()
    others = [i for i in range(3) if i != v]
    assert not m[others].any() and not tr.exposure_exp_avg_sq.cpu().numpy()[others].any()
    assert torch.equal(tr.exposure[others], start[others])
    assert not torch.equal(tr.exposure[v], start[v]) and tr.exposure_step == 1
    # ---- the Gaussians received the exposure's dL/dimage
    sc_, q_, o_ = T.activate(s.raw_scales, s.raw_rotations, s.raw_opacities.reshape(-1, 1))
    f = oracle.forward(cam, s.means3D, o_.reshape(-1), sh_dc=s.sh_dc, sh_rest=s.sh_rest, sh_degree=3, scales=sc_,
                       rotations=q_)
    g = f.state.backward(ref["dimg"].astype(f32))
    mx = tr.exp_avg["xyz"].cpu().numpy()
    r = rel_l2(mx, 0.1 * np.asarray(g["means3D"], np.float64).reshape(mx.shape))
    print("exp_avg[xyz] rel_l2", r)
    assert r <= 1e-4, r
    # ---- step 2 on another view: the whole tensor steps
    g1 = torch.zeros(3, 3, 4, dtype=dt)
    g1[v] = out["dL_dexposure"].cpu().to(dt)
    after1 = tr.exposure.clone()
    out2 = tr.step(2, cam, _t(gt), densify=False, view_index=u)
    g2 = torch.zeros(3, 3, 4, dtype=dt)
    g2[u] = out2["dL_dexposure"].cpu().to(dt)
    p = start.cpu().to(dt).requires_grad_(True)
    adam = torch.optim.Adam([p], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    for it, grad in ((1, g1), (2, g2)):
        adam.param_groups[0]["lr"] = tr.exposure_scheduler(it)
        p.grad = grad.clone()
        adam.step()
    got, want = tr.exposure.cpu().numpy().astype(np.float64), p.detach().numpy()
    moved = np.abs(got[v] - after1[v].cpu().numpy()).min()
    err = np.abs(got - want).max()
    print("whole-tensor Adam: rel_l2", rel_l2(got, want), "max err / max", err / np.abs(want).max(),
          "row v's smallest second move", moved)
    assert moved > 1e-3  # row v moved again without a gradient
    assert rel_l2(got, want) <= 1e-6 and err <= 1e-6 * np.abs(want).max()
    assert torch.equal(tr.exposure[0], start[0]) and tr.exposure_step == 2


# ---------------------------------------------------------------------------------------------
# 8 - 9. learning, checkpoints, the loop
# ---------------------------------------------------------------------------------------------
N_GT = 4000
FROZEN = dict(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0,
              rotation_lr=0.0)


def _gt_trainer(scene, leaves, **opt):
    Tr = pkg("trainer")
    xyz, f_dc, f_rest, opac, log_s, q = leaves
    return Tr.GaussianTrainer(xyz, f_dc, f_rest, opac, log_s, q, max_sh_degree=1, opt=Tr.OptimizationParams(**opt),
                              spatial_lr_scale=scene.extent, device=DEV)


def test_it_learns_the_exposure(K):
    """One 64 x 64 view of the ground-truth cloud with every Gaussian LR 0; the target is the render
    under E_TRUE (clamped).  100 iterations at the default exposure LRs: the L1 stat falls to at
    most 1/4 of iteration 1's and mean |E - E_TRUE| to at most 1/4 of its initial value -- a
    condition a wrong gradient (transposed 3 x 3 part, dropped bias, wrong sign) cannot meet, not a
    measurement.  The fp64 torch restatement of this case on the CPU (the oracle's render of the same
    cloud, 0.8 L1 + 0.2 D-SSIM, torch.optim.Adam) reaches 0.074 and 0.028; the measured ratios are in
    DESIGN.md section 9f."""
    L = pkg("train_loop")
    scene = L.synthetic_scene(N_GT, 500, 1, 64, 64, seed=0, device=DEV, gt_scale=0.05)
    leaves = L.procedural_cloud(N_GT, 0, 0.25, 0.05)[:6]
    tr = _gt_trainer(scene, leaves, train_exposure=True, iterations=30000, **FROZEN)
    tr.setup_exposure(1)
    cam = scene.cams[0]
    target = K.exposure_forward(tr.render(cam).color.contiguous(), _t(E_TRUE), clamp=True)
    xyz0 = tr.params["xyz"].clone()
    d0 = float((tr.exposure[0].cpu() - torch.tensor(E_TRUE)).abs().mean())
    l1 = {}
    for it in range(1, 101):
        out = tr.step(it, cam, target, densify=False, view_index=0)
        if it in (1, 100):
            l1[it] = out["stats"][1].clone()
    d1 = float((tr.exposure[0].cpu() - torch.tensor(E_TRUE)).abs().mean())
    first, last = float(l1[1]), float(l1[100])
    print("L1 first", first, "last", last, "ratio", last / first, "| mean |E - E_true|", d0, "->", d1, "ratio", d1 / d0)
    assert torch.equal(tr.params["xyz"], xyz0)  # the Gaussians stood still
    assert first > 0 and last <= first / 4
    assert d1 <= d0 / 4


def test_checkpoint_carries_the_exposure(step_scene, tmp_path):
    cam, s, gt = (step_scene[k] for k in ("cam", "s", "gt"))
    tr = _trainer(s, train_exposure=True)
    tr.setup_exposure(3, names=["a.png", "b.png", "c.png"])
    for it, view in ((1, 2), (2, 0)):
        tr.step(it, cam, _t(gt), densify=False, view_index=view)
    path = str(tmp_path / "chkpnt.pth")
    tr.capture(path)
    other = _trainer(s, train_exposure=True)
    assert other.exposure is None
    other.restore(path)
    assert torch.equal(other.exposure, tr.exposure) and other.exposure.is_cuda and other.exposure.is_contiguous()
    assert torch.equal(other.exposure_exp_avg, tr.exposure_exp_avg)
    assert torch.equal(other.exposure_exp_avg_sq, tr.exposure_exp_avg_sq)
    assert other.exposure_step == tr.exposure_step == 2 and other.exposure_names == ["a.png", "b.png", "c.png"]
    assert not torch.equal(tr.exposure[2], torch.eye(3, 4, device=DEV))
    # the restored trainer continues as the original does
    oa = tr.step(3, cam, _t(gt), densify=False, view_index=1)
    ob = other.step(3, cam, _t(gt), densify=False, view_index=1)
    assert torch.equal(oa["dL_dexposure"], ob["dL_dexposure"]) and torch.equal(tr.exposure, other.exposure)
    # exposure.json
    jpath = str(tmp_path / "exposure.json")
    tr.save_exposures(jpath)
    back = pkg("scene_io").load_exposures(jpath)
    assert list(back) == ["a.png", "b.png", "c.png"]
    assert all(np.array_equal(back[n], tr.exposure[i].cpu().numpy()) for i, n in enumerate(back))
    # a checkpoint without exposure restores and leaves it unset
    plain = _trainer(s)
    plain.step(1, cam, _t(gt), densify=False)
    ppath = str(tmp_path / "plain.pth")
    plain.capture(ppath)
    other.restore(ppath)
    assert other.exposure is None and other.exposure_names is None
    assert torch.equal(other.params["xyz"], plain.params["xyz"])


def test_train_loop_trains_the_exposure():
    """train() over 24 views with per-view exposures in the targets, 20 iterations: step() gets the
    view's index, the rows of the views visited (before the last iteration, which takes no optimizer
    step) move, the others stay eye(3, 4) with zero moments."""
    L, Tr = pkg("train_loop"), pkg("trainer")
    n_views, W, H = 24, 96, 64
    rng = np.random.default_rng(3)
    exposures = [np.eye(3, 4, dtype=f32) if i == 0 else
                 (np.eye(3, 4) + rng.uniform(-0.05, 0.05, (3, 4))).astype(f32) for i in range(n_views)]
    scene = L.synthetic_scene(N_GT, 500, n_views, W, H, seed=0, device=DEV, gt_scale=0.05, exposures=exposures)
    plain = L.synthetic_scene(N_GT, 500, n_views, W, H, seed=0, device=DEV, gt_scale=0.05)
    assert plain.exposures is None and len(scene.exposures) == n_views
    assert all(np.array_equal(a, b) for a, b in zip(scene.exposures, exposures))
    k = Tr.TrainKernels(DEV)
    assert torch.equal(scene.gts[0], plain.gts[0])  # the identity leaves a target in [0, 1] as it was
    assert torch.equal(scene.gts[1], k.exposure_forward(plain.gts[1], _t(exposures[1]), clamp=True))
    assert not torch.equal(scene.gts[1], plain.gts[1])
    opt = Tr.OptimizationParams(iterations=20, train_exposure=True)
    res = L.train(scene, opt=opt, max_sh_degree=1, log_every=10, device=DEV)
    assert res.iterations == 20 and res.binning_overflows == 0
    assert {"exposed", "dL_dexposure", "image"} <= set(res.last_step)
    tr = res.trainer
    assert tr.exposure.shape == (n_views, 3, 4) and tr.exposure_step == 19
    visited = set(int(v) for v in L.view_sequence(n_views, 20, 0)[:19])
    assert 0 < len(visited) < n_views
    eye = torch.eye(3, 4, device=DEV)
    for i in range(n_views):
        if i in visited:
            assert not torch.equal(tr.exposure[i], eye), i
            assert bool(tr.exposure_exp_avg_sq[i].abs().sum() > 0), i
        else:
            assert torch.equal(tr.exposure[i], eye), i
            assert not tr.exposure_exp_avg[i].any() and not tr.exposure_exp_avg_sq[i].any(), i
    assert L.train(plain, opt=Tr.OptimizationParams(iterations=2), max_sh_degree=1, log_every=1,
                   device=DEV).trainer.exposure is None
