"""GPU: MCMC densification (gsr_mcmc_relocate, gsr_mcmc_noise; TrainKernels.mcmc_relocate / mcmc_noise;
OptimizationParams.densify_strategy = "mcmc", GaussianTrainer.mcmc_refine).

The kernels are compared with the fp64 restatements of tests/mcmc_reference.py.

Relocation: the kernel evaluates x, D and o / D in fp64 and rounds once, so it is held to the fp64
reference rounded to fp32 at 4 x 2^-24 relative (fp64 evaluation is good to 2e-12, one rounding to fp32
costs 2^-24, the factor 4 covers the device's pow / sqrt differing from the host's in the last places
of a double).

Noise: the gate multiplies any error in o by 100, so an fp32 chain cannot be held to a few ulps of the
fp64 value; the bound is measured instead: e_ref = the largest norm-wise relative error, over the
Gaussians, of the same formula written with torch fp32 ops on the device, and the kernel's largest
error must be at most 4 e_ref (operation order, fused multiply-adds).  Measured on an MI355X:
e_ref = 1.282e-5, kernel 3.436e-6.

Everything the specification makes exact is compared with torch.equal."""
import numpy as np
import pytest
import torch

import mcmc_reference as ref
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
STRENGTH = 5e5 * 1.6e-4
P = 1027  # several waves and a tail
GATE_OPACITIES = (0.001, 0.004, 0.005, 0.006, 0.01, 0.03, 0.1)


@pytest.fixture(scope="module")
def K():
    return pkg("trainer").TrainKernels(DEV)


def _logit(o):
    o = np.asarray(o, np.float64)
    return np.log(o / (1.0 - o)).astype(np.float32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


# ---------------------------------------------------------------- 1. relocation
def test_relocation_value(K):
    n = P
    o = np.minimum(np.geomspace(0.005, 1.0 - EPS, n), 1.0 - EPS).astype(np.float32)
    assert o[-1] == np.float32(1.0 - EPS) and o[0] == np.float32(0.005)
    ratios = np.array([1 + i % 51 for i in range(n - 4)] + [0, -3, 52, 1000], np.int32)
    scales = np.exp(np.random.default_rng(0).uniform(-6.0, 0.0, (n, 3))).astype(np.float32)
    new_o, new_s = K.mcmc_relocate(_dev(o), _dev(scales), _dev(ratios), 0.005)
    new_o, new_s = new_o.cpu().numpy(), new_s.cpu().numpy()
    ref_o, ref_s = ref.relocate(o, scales, ratios, 0.005)
    assert [ref.clamp_ratio(r) for r in ratios[-4:]] == [1, 1, 51, 51]
    err_o = np.abs(new_o.astype(np.float64) - ref_o.astype(np.float32)) / np.abs(ref_o)
    err_s = np.abs(new_s.astype(np.float64) - ref_s.astype(np.float32)) / np.abs(ref_s)
    print(f"relocation: worst relative error opacity {err_o.max() / EPS:.2f} x 2^-24, "
          f"scale {err_s.max() / EPS:.2f} x 2^-24")
    assert err_o.max() <= 4 * EPS, (int(err_o.argmax()), err_o.max())
    assert err_s.max() <= 4 * EPS, (int(err_s.argmax()), err_s.max())
    assert new_o.min() >= np.float32(0.005) and new_o.max() <= np.float32(1.0 - EPS)
    # the out-of-range ratios act as their clamped values on the same rows
    again_o, again_s = K.mcmc_relocate(_dev(o[-4:]), _dev(scales[-4:]), _dev(np.array([1, 1, 51, 51], np.int32)), 0.005)
    assert np.array_equal(again_o.cpu().numpy(), new_o[-4:]) and np.array_equal(again_s.cpu().numpy(), new_s[-4:])


# ---------------------------------------------------------------- 2 - 5. noise
@pytest.fixture(scope="module")
def noise_inputs():
    rng = np.random.default_rng(1)
    scale_raw = rng.uniform(-6.0, 0.0, (P, 3)).astype(np.float32)
    q = rng.standard_normal((P, 4))
    q *= (10.0 ** rng.uniform(-1.0, 1.0, (P, 1))) / np.linalg.norm(q, axis=1, keepdims=True)  # norms in [0.1, 10]
    opac_raw = _logit([GATE_OPACITIES[i % len(GATE_OPACITIES)] for i in range(P)]).reshape(P, 1)
    noise = rng.standard_normal((P, 3)).astype(np.float32)
    host = dict(scale_raw=scale_raw, rot_raw=q.astype(np.float32), opac_raw=opac_raw, noise=noise)
    return host, {k: _dev(v) for k, v in host.items()}


def _run_noise(K, d, xyz, guard=None, strength=STRENGTH):
    out = xyz.clone()
    K.mcmc_noise(out, d["scale_raw"], d["rot_raw"], d["opac_raw"], d["noise"], strength, guard=guard)
    return out


@pytest.fixture(scope="module")
def displacement(K, noise_inputs):
    """The kernel on xyz = 0: the output is the displacement."""
    _, d = noise_inputs
    return _run_noise(K, d, torch.zeros((P, 3), device=DEV))


def _torch_fp32_displacement(d):
    """The header's formula with torch fp32 ops on the device."""
    general = pkg("general")
    s = torch.exp(d["scale_raw"])
    q = d["rot_raw"] / torch.clamp_min(torch.linalg.norm(d["rot_raw"], dim=1, keepdim=True), 1e-12)
    R = general.build_rotation(q)
    o = torch.sigmoid(d["opac_raw"])
    gate = 1.0 / (1.0 + torch.exp(100.0 * (o - 0.005)))
    sigma = R @ ((s * s)[:, :, None] * R.transpose(1, 2))
    return (sigma @ (d["noise"] * gate * STRENGTH)[:, :, None])[:, :, 0]


def _worst_rel(a, b):
    return float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())


def test_noise_value(K, noise_inputs, displacement):
    host, d = noise_inputs
    want = ref.noise_displacement(host["scale_raw"], host["rot_raw"], host["opac_raw"], host["noise"], STRENGTH)
    gates = ref.noise_gate(host["opac_raw"])
    assert gates.min() < 1e-4 and gates.max() > 0.59  # the gate covers its range
    e_ref = _worst_rel(_torch_fp32_displacement(d).cpu().numpy().astype(np.float64), want)
    e_kernel = _worst_rel(displacement.cpu().numpy().astype(np.float64), want)
    print(f"noise: worst norm-wise relative error, torch fp32 {e_ref:.3e}, kernel {e_kernel:.3e}")
    assert e_ref < 1e-3  # the yardstick itself is an fp32 evaluation of the same formula
    assert e_kernel <= 4 * e_ref, (e_kernel, e_ref)


def test_noise_add(K, noise_inputs, displacement):
    _, d = noise_inputs
    gen = torch.Generator(device=DEV)
    gen.manual_seed(2)
    xyz = 3.0 * torch.randn((P, 3), generator=gen, device=DEV)
    out = _run_noise(K, d, xyz)
    want = xyz + displacement
    lo = torch.nextafter(want, torch.full_like(want, -float("inf")))
    hi = torch.nextafter(want, torch.full_like(want, float("inf")))
    assert bool(((out >= lo) & (out <= hi)).all())
    assert not torch.equal(out, xyz)


def test_opaque_rows_are_untouched(K, noise_inputs):
    _, d = noise_inputs
    opaque = (0.5, 0.999, 1.0 - EPS)
    o = [opaque[i % 3] if i % 2 == 0 else 0.004 for i in range(P)]
    d = dict(d, opac_raw=_dev(_logit(o).reshape(P, 1)))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    xyz = 3.0 * torch.randn((P, 3), generator=gen, device=DEV)
    out = _run_noise(K, d, xyz)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[0::2], xyz[0::2])
    assert bool((out[1::2] != xyz[1::2]).any(dim=1).all())  # the transparent rows in between did move


def test_noise_guard_and_determinism(K, noise_inputs):
    _, d = noise_inputs
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    xyz = 3.0 * torch.randn((P, 3), generator=gen, device=DEV)
    cap = 1000
    free = _run_noise(K, d, xyz)
    assert torch.equal(free, _run_noise(K, d, xyz))
    assert not torch.equal(free, xyz)
    tripped = _run_noise(K, d, xyz, guard=(torch.tensor([cap + 1], dtype=torch.int32, device=DEV), cap))
    assert torch.equal(tripped, xyz)
    passed = _run_noise(K, d, xyz, guard=(torch.tensor([cap], dtype=torch.int32, device=DEV), cap))
    assert torch.equal(passed, free)
    assert torch.equal(_run_noise(K, d, xyz, strength=0.0), xyz)


# ---------------------------------------------------------------- 6 - 9. the trainer
@pytest.fixture(scope="module")
def scene():
    return pkg("train_loop").synthetic_scene(n_gt=2000, n_init=400, n_views=4, width=64, height=64, seed=5, device=DEV)


def _all_tensors(tr):
    T = pkg("trainer")
    return [d[k] for d in (tr.params, tr.exp_avg, tr.exp_avg_sq) for k in T.GROUPS]


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(_all_tensors(a), _all_tensors(b)))


def _scene_trainer(scene, seed=0, **opt_kw):
    T = pkg("trainer")
    return T.GaussianTrainer.from_point_cloud(scene.points, scene.colors, 1, spatial_lr_scale=scene.extent,
                                              opt=T.OptimizationParams(**opt_kw), device=DEV, seed=seed)


def test_trainer_count_schedule(scene):
    tr = _scene_trainer(scene, densify_strategy="mcmc", cap_max=450, densify_from_iter=0, densification_interval=5)
    assert tr.num_points == 400
    counts, ptrs = [], []
    for it in range(1, 26):
        v = it % len(scene.cams)
        out = tr.step(it, scene.cams[v], scene.gts[v])
        assert tr.num_points <= 450 and out["num_points"] == tr.num_points
        if it % 5 == 0:
            counts.append(tr.num_points)
            ptrs.append([t.data_ptr() for t in _all_tensors(tr)])
    assert counts == [420, 441, 450, 450, 450]
    assert len(ptrs[2]) == 18 and ptrs[2] == ptrs[3] == ptrs[4]  # never reallocated once at cap_max
    assert all(bool(torch.isfinite(t).all()) for t in _all_tensors(tr))


def _hand_trainer(seed=0):
    """300 rows, 40 of them dead (raw opacity -8), non-zero moments everywhere, no room to grow."""
    T = pkg("trainer")
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    n = 300
    r = lambda *shape: torch.randn(shape, generator=gen)
    opacity = r(n, 1)
    dead = torch.randperm(n, generator=gen)[:40]
    opacity[dead] = -8.0
    tr = T.GaussianTrainer(r(n, 3), r(n, 1, 3), r(n, 3, 3), opacity, r(n, 3) - 3.0, r(n, 4), max_sh_degree=1,
                           opt=T.OptimizationParams(densify_strategy="mcmc", cap_max=n), device=DEV, seed=seed)
    for k in T.GROUPS:
        tr.exp_avg[k].copy_(r(*tr.params[k].shape) * 1e-2 + 1.0)
        tr.exp_avg_sq[k].copy_(r(*tr.params[k].shape) ** 2 + 1e-3)
    return tr, torch.sort(dead).values.to(DEV)


def test_refine_invariants():
    T = pkg("trainer")
    tr, dead = _hand_trainer()
    n = tr.num_points
    before = [t.clone() for t in _all_tensors(tr)]
    ptrs = [t.data_ptr() for t in _all_tensors(tr)]
    info = tr.mcmc_refine()
    assert info == {"relocated": 40, "added": 0} and tr.num_points == n
    assert ptrs == [t.data_ptr() for t in _all_tensors(tr)]  # rows written in place
    assert float(torch.sigmoid(tr.params["opacity"]).min()) >= tr.opt.mcmc_min_opacity - 1e-6
    live = torch.ones(n, dtype=torch.bool, device=DEV)
    live[dead] = False
    live_idx = torch.nonzero(live)[:, 0]
    # every formerly dead row is a copy of one formerly live row, in all six parameters
    match = (tr.params["xyz"][dead][:, None, :] == tr.params["xyz"][live_idx][None, :, :]).all(dim=2)
    assert bool(match.any(dim=1).all())
    src = live_idx[match.to(torch.int32).argmax(dim=1)]
    for k in T.GROUPS:
        assert torch.equal(tr.params[k][dead], tr.params[k][src]), k
    # moments: zero on exactly the source rows, bit-unchanged elsewhere (the dead rows keep theirs)
    is_src = torch.zeros(n, dtype=torch.bool, device=DEV)
    is_src[src] = True
    assert 0 < int(is_src.sum()) <= 40
    params0, m0, v0 = before[:6], before[6:12], before[12:]
    for i, k in enumerate(T.GROUPS):
        for now, was in ((tr.exp_avg[k], m0[i]), (tr.exp_avg_sq[k], v0[i])):
            assert bool((now[is_src] == 0).all()), k
            assert torch.equal(now[~is_src], was[~is_src]), k
            assert bool((was != 0).all())
        untouched = live & ~is_src  # live rows nobody was relocated onto keep their parameters
        assert torch.equal(tr.params[k][untouched], params0[i][untouched]), k
    # the sources gave up opacity: they now share their place
    o_now, o_was = torch.sigmoid(tr.params["opacity"][is_src]), torch.sigmoid(params0[3][is_src])
    assert bool((o_now <= o_was).all())
    # a seed reproduces the refinement bit for bit
    again, _ = _hand_trainer()
    again.mcmc_refine()
    assert _same_state(tr, again)


def _pair(scene, a_kw, b_kw):
    a, b = _scene_trainer(scene, **a_kw), _scene_trainer(scene, **b_kw)
    assert _same_state(a, b)
    return a, b


def test_step_without_noise_and_regularisers_is_the_default_step(scene):
    a, b = _pair(scene, dict(densify_strategy="mcmc", noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0), dict())
    for it in range(1, 4):
        v = it % len(scene.cams)
        oa = a.step(it, scene.cams[v], scene.gts[v])
        ob = b.step(it, scene.cams[v], scene.gts[v], densify=False)
        assert torch.equal(oa["stats"], ob["stats"])
    assert _same_state(a, b)


def test_step_is_the_composition_of_the_public_pieces(scene):
    T = pkg("trainer")
    a, b = _pair(scene, dict(densify_strategy="mcmc"), dict(densify_strategy="mcmc"))
    quiet = _scene_trainer(scene, densify_strategy="mcmc", noise_lr=0.0)
    cam, gt, it = scene.cams[1], scene.gts[1], 1
    a.step(it, cam, gt)
    quiet.step(it, cam, gt)
    opt = b.opt
    b.update_learning_rate(it)
    st = b.render(cam)
    _, maps = b.k.loss_forward(st.color, gt, opt.lambda_dssim)
    dimg = b.k.loss_backward(st.color, gt, opt.lambda_dssim, maps)
    g = b.rast.backward(st, dimg)
    n = b.num_points
    g["opacities"].add_(opt.opacity_reg / n)
    g["scales"].add_(opt.scale_reg / (3 * n))
    b.optimizer_step({"xyz": g["means3D"], "f_dc": g["sh_dc"], "f_rest": g["sh_rest"], "opacity": g["opacities"],
                      "scaling": g["scales"], "rotation": g["rotations"]})
    noise = torch.randn((n, 3), dtype=torch.float32, device=DEV, generator=b.gen)
    b.k.mcmc_noise(b.params["xyz"], b.params["scaling"], b.params["rotation"], b.params["opacity"], noise,
                   opt.noise_lr * b.lr["xyz"], guard=b._guard)
    assert _same_state(a, b)
    assert all(a.steps[k] == b.steps[k] == 1 for k in T.GROUPS)
    assert not torch.equal(a.params["xyz"], quiet.params["xyz"])  # the noise did move the means
    vals = a.regularizer_values()
    assert vals["opacity_reg"] == pytest.approx(opt.opacity_reg * float(torch.sigmoid(a.params["opacity"]).mean()))
    assert vals["scale_reg"] == pytest.approx(opt.scale_reg * float(torch.exp(a.params["scaling"]).mean()))


def test_short_run_is_sane(scene):
    """A sanity condition, not a parity claim."""
    T, loop = pkg("trainer"), pkg("train_loop")
    opt = T.OptimizationParams(densify_strategy="mcmc", cap_max=600, densify_from_iter=0, densification_interval=20)
    res = loop.train(scene, iterations=300, opt=opt, max_sh_degree=1, log_every=1, device=DEV)
    losses = [l for _, l, _, _ in res.loss]
    assert len(losses) >= 300 and all(np.isfinite(losses))
    first, last = float(np.mean(losses[:20])), float(np.mean(losses[-20:]))
    print(f"loss: first 20 {first:.4f}, last 20 {last:.4f}; points {res.final_points}, peak {res.peak_points}")
    assert last < first
    assert res.final_points <= 600 and res.peak_points <= 600
    assert [c for _, c in res.num_points][:3] == [420, 441, 463]
    assert res.binning_overflows == 0
