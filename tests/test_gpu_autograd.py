"""The libtorch RasterizeGaussians autograd Function (C++ render() surface) on the GPU:
its gradients equal the C-ABI backward, and render() with a GaussianModel trains."""
import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

pytestmark = pytest.mark.gpu


def _setup(P=4000, W=192, H=144, seed=3):
    gr, sc = pkg("graphics"), pkg("scene")
    cam = gr.synthetic_camera(W, H)
    return cam, sc.make_scene(cam, P, max_sh_degree=3, seed=seed), sc.make_dL_dpix(cam, seed=seed + 1)


def test_autograd_matches_cabi():
    cam, s, dpix = _setup()
    R = pkg("rasterizer")
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)
    means, opac, scales, rots, dc, rest = (t(s.means3D), t(s.opacities), t(s.scales), t(s.rotations),
                                           t(s.sh_dc), t(s.sh_rest))
    m2d = torch.zeros_like(means, requires_grad=True)
    color, radii = R.rasterize_gaussians(cam, means, m2d, opac, sh_dc=dc, sh_rest=rest, scales=scales,
                                         rotations=rots, sh_degree=3)
    (color * torch.tensor(dpix, device=dev)).sum().backward()
    cabi = R.CAbiRasterizer(dev)
    st = cabi.forward(cam, s.means3D, s.opacities, s.scales, s.rotations, s.sh_dc, s.sh_rest, sh_degree=3)
    assert torch.equal(st.color, color.detach())
    assert torch.equal(st.radii, radii)
    g = cabi.backward(st, dpix)
    pairs = dict(means3D=means, opacities=opac, scales=scales, rotations=rots, sh_dc=dc, sh_rest=rest,
                 means2D=m2d)
    for k, leaf in pairs.items():
        assert torch.equal(leaf.grad.reshape(g[k].shape), g[k]), k


def test_render_with_model_and_pipeline_flags():
    cam, s, dpix = _setup(P=3000)
    R, M = pkg("rasterizer"), pkg("model")
    model = M.GaussianModel.from_scene(s, "cuda")
    bg = torch.zeros(3, device="cuda")
    base = R.render(cam, model, R.PipelineParams(), bg)
    assert base["render"].shape == (3, cam.height, cam.width)
    assert torch.equal(base["visibility_filter"], base["radii"] > 0)
    # compute_cov3D_python and convert_SHs_python select the precomputed paths: same image
    alt = R.render(cam, model, R.PipelineParams(convert_SHs_python=True, compute_cov3D_python=True), bg)
    assert rel_l2(alt["render"].detach().cpu().numpy(), base["render"].detach().cpu().numpy()) < 1e-4
    # gradients reach every leaf through the activations, and a few Adam steps lower an L2 loss
    target = torch.rand_like(base["render"])
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        out = R.render(cam, model, R.PipelineParams(), bg)
        loss = ((out["render"] - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        assert out["viewspace_points"].grad is not None
        losses.append(float(loss))
        opt.step()
    assert losses[-1] < losses[0]
    for p in model.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def test_precomputed_inputs_autograd():
    cam, s, dpix = _setup(P=1500)
    R, general = pkg("rasterizer"), pkg("general")
    dev = "cuda"
    means = torch.tensor(s.means3D, device=dev, requires_grad=True)
    cov = general.build_covariance_from_scaling_rotation(torch.tensor(s.scales, device=dev), 1.0,
                                                         torch.tensor(s.rotations, device=dev))
    cov = cov.detach().requires_grad_(True)
    cols = torch.rand((s.P, 3), device=dev, requires_grad=True)
    opac = torch.tensor(s.opacities, device=dev, requires_grad=True)
    m2d = torch.zeros_like(means, requires_grad=True)
    color, radii = R.rasterize_gaussians(cam, means, m2d, opac, colors_precomp=cols, cov3D_precomp=cov)
    (color * torch.tensor(dpix, device=dev)).sum().backward()
    for leaf in (means, cov, cols, opac, m2d):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all())
    assert float(cov.grad.abs().sum()) > 0


# ---- caller-visible gradient shapes (the C++ layer's one LeafGrads behind both paths) ----
_P, _W, _H = 257, 48, 32  # one 256-Gaussian block plus one


@pytest.fixture(scope="module")
def small():
    gr, sc, general = pkg("graphics"), pkg("scene"), pkg("general")
    cam = gr.synthetic_camera(_W, _H)
    s = sc.make_scene(cam, _P, max_sh_degree=1, seed=5)
    assert s.sh_rest.reshape(_P, -1, 3).shape[1] == 3
    cov = general.build_covariance_from_scaling_rotation(torch.tensor(s.scales, device="cuda"), 1.0,
                                                         torch.tensor(s.rotations, device="cuda")).detach()
    cols = torch.rand((_P, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    return cam, s, torch.tensor(sc.make_dL_dpix(cam, seed=7), device="cuda"), cov.reshape(_P, 6).contiguous(), cols


def _shape_case(case, small):
    """-> (inputs of the case as device tensors by ShardStep's key names, sh_degree)."""
    cam, s, dpix, cov, cols = small
    t = lambda a, *shape: torch.tensor(a, device="cuda").reshape(*shape).contiguous()
    if case == "precomp":
        return dict(means3D=t(s.means3D, _P, 3), opacities=t(s.opacities, _P), colors_precomp=cols.clone(),
                    cov3D_precomp=cov.clone()), 0
    opac = t(s.opacities, _P) if case == "sh-opacity-P" else t(s.opacities, _P, 1)
    return dict(means3D=t(s.means3D, _P, 3), opacities=opac, scales=t(s.scales, _P, 3),
                rotations=t(s.rotations, _P, 4), sh_dc=t(s.sh_dc, _P, 1, 3), sh_rest=t(s.sh_rest, _P, 3, 3)), 1


_CASES = ["sh-opacity-P", "sh-opacity-Px1", "precomp"]


@pytest.mark.parametrize("case", _CASES)
def test_autograd_gradient_shapes(case, small):
    """rasterize_gaussians returns every gradient in its input's own shape (opacities as (P,) or
    (P,1), sh_dc (P,1,3), sh_rest (P,3,3), ...), None for the absent inputs, and (P,3) for means2D."""
    cam, s, dpix, _, _ = small
    R = pkg("rasterizer")
    inputs, D = _shape_case(case, small)
    leaves = {k: v.requires_grad_(True) for k, v in inputs.items()}
    m2d = torch.zeros((_P, 3), device="cuda", requires_grad=True)
    kw = {k: v for k, v in leaves.items() if k not in ("means3D", "opacities")}
    color, radii = R.rasterize_gaussians(cam, leaves["means3D"], m2d, leaves["opacities"], sh_degree=D, **kw)
    args = [leaves["means3D"], m2d] + [leaves[k] for k in leaves if k != "means3D"]
    grads = torch.autograd.grad((color * dpix).sum(), args, allow_unused=True)
    for a, g in zip(args, grads):
        assert g is not None and g.shape == a.shape and g.dtype == torch.float32
    assert grads[1].shape == (_P, 3)
    # the absent optional inputs: the Function's backward hands autograd no gradient for them
    ext = pkg("native").load_torch_ext()
    order = ("sh_dc", "sh_rest", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
    full = [leaves[k] if k in leaves else torch.empty(0, device="cuda", requires_grad=True) for k in order]
    out = ext.rasterize_gaussians(R.ext_camera(cam), R._ext_settings(ext, (0.0, 0.0, 0.0), 1.0, D, None, False, 0),
                                  leaves["means3D"], m2d, *full)
    got = torch.autograd.grad((out[0] * dpix).sum(), [leaves["means3D"], m2d] + full, allow_unused=True)
    for k, a, g in zip(order, full, got[2:]):
        assert (g is None) == (k not in leaves), k
        assert g is None or g.shape == a.shape, k


@pytest.mark.parametrize("case", _CASES)
def test_shard_step_gradient_shapes_and_bits(case, small):
    """ext.ShardStep over a world-1 RCCL exchange (graph off): the grads dict has exactly the
    canonical keys and shapes, and its values are the single-GPU CAbiRasterizer.backward gradients
    bit for bit (one band: the same blend order)."""
    cam, s, dpix, _, _ = small
    R = pkg("rasterizer")
    ext = pkg("native").load_torch_ext()
    inputs, D = _shape_case(case, small)
    ex = ext.rccl_exchange(ext.rccl_unique_id(), 0, 1)
    step = ext.ShardStep(ex, R.ext_camera(cam), inputs, D, graph=False)
    step.plan()
    image, grads, radii = step.step(dpix)
    step.check()
    M = 3
    want = dict(means2D=(_P, 3), conic=(_P, 3), opacities=(_P, 1), means3D=(_P, 3))
    if case == "precomp":
        want.update(colors=(_P, 3), cov3D=(_P, 6))
    else:
        want.update(sh_dc=(_P, 1, 3), sh_rest=(_P, M, 3), scales=(_P, 3), rotations=(_P, 4))
    assert {k: tuple(v.shape) for k, v in grads.items()} == want
    cabi = R.CAbiRasterizer("cuda")
    st = cabi.forward(cam, inputs["means3D"], inputs["opacities"], inputs.get("scales"), inputs.get("rotations"),
                      inputs.get("sh_dc"), inputs.get("sh_rest"), sh_degree=D,
                      colors_precomp=inputs.get("colors_precomp"), cov3D_precomp=inputs.get("cov3D_precomp"))
    ref = cabi.backward(st, dpix)
    assert torch.equal(image, st.color) and torch.equal(radii, st.radii)
    assert set(ref) == set(want)
    for k in want:
        assert tuple(ref[k].shape) == want[k] and torch.equal(grads[k], ref[k]), k
