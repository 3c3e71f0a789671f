"""float64 reference for the camera gradients (TEST INFRASTRUCTURE).

A restatement of dense_reference.preprocess whose camera fields are autograd leaves expanded to one
row per Gaussian -- V (P, 16), Pm (P, 16), campos (P, 3), every row the camera's values -- so that after
a backward the rows of their .grad are the per-Gaussian terms of dL/dviewmatrix, dL/dprojmatrix and
dL/dcampos: their column sums are the reference gradient, the column sums of their magnitudes the scale
the kernels' f32 summation error is measured against.  It adds what dense_reference.preprocess has not:
the anti-aliased opacity o' = o sqrt(max(0.000025, det0 / det)) and the depth channel's value
v = tz (or 1 / tz).  The three fields are independent inputs, exactly as the kernels read them.
dense_reference.render, geometry_f32 and sh_basis are reused by import.

It is also the float64 reference of the leaf gradients on the edge scene (make_case(edge=True),
tests/test_edge_reference.py): float64 leaf tensors passed as inputs stay in the graph, and
band_grad="upstream" gives B2's convention outside the guard band instead of the camera kernel's.
"""
from __future__ import annotations

import torch

from dense_reference import geometry_f32, render, sh_basis  # noqa: F401  (render, geometry_f32: re-exported)

DT = torch.float64


def t64(a):
    return None if a is None else torch.as_tensor(a, dtype=DT)


def preprocess(cam, means, opac, scales=None, rots=None, sh_dc=None, sh_rest=None, D=0, colors=None, cov3D=None,
               scale_mod=1.0, antialias=False, inverse_depth=False, band_grad="forward"):
    """The per-Gaussian quantities the blend consumes, differentiable in the expanded camera leaves
    "V", "Pm", "campos" (returned in the dict) and in any float64 leaf passed as an input.  Keys as
    dense_reference.preprocess (xy, depth, conic, opacity, rgb) plus "ndc", "value" (the depth channel's
    v), "sh_sum" (res before the clamp, or None) and "txtz" / "tytz" (the guard-band arguments).

    band_grad: the derivative of J's cx = clamp(tx / tz, +-1.3 tan(fov)) tz (and cy) outside the guard
    band.  "forward": the forward's own (cx = +-lim tz, dJ02/dtz = fx cx / tz^3), what the camera kernel
    computes.  "upstream": the clamped cx a constant (dL/dtx gets nothing, dJ02/dtz keeps the in-band
    2 fx cx / tz^3), what B2 and the CPU oracle compute.  The values are the same."""
    if band_grad not in ("forward", "upstream"):
        raise ValueError(f"band_grad: {band_grad!r}")
    means, opac, scales, rots, sh_dc, sh_rest, colors, cov3D = (t64(a) for a in (means, opac, scales, rots, sh_dc,
                                                                                 sh_rest, colors, cov3D))
    P = means.shape[0]
    leaf = lambda a, n: torch.tensor(a, dtype=DT).reshape(1, n).repeat(P, 1).requires_grad_(True)
    V, Pm, cp = leaf(cam.viewmatrix, 16), leaf(cam.projmatrix, 16), leaf(cam.campos, 3)
    x, y, z = means[:, 0], means[:, 1], means[:, 2]
    tx = V[:, 0] * x + V[:, 4] * y + V[:, 8] * z + V[:, 12]
    ty = V[:, 1] * x + V[:, 5] * y + V[:, 9] * z + V[:, 13]
    tz = V[:, 2] * x + V[:, 6] * y + V[:, 10] * z + V[:, 14]
    hx = Pm[:, 0] * x + Pm[:, 4] * y + Pm[:, 8] * z + Pm[:, 12]
    hy = Pm[:, 1] * x + Pm[:, 5] * y + Pm[:, 9] * z + Pm[:, 13]
    hw = Pm[:, 3] * x + Pm[:, 7] * y + Pm[:, 11] * z + Pm[:, 15]
    pw = 1.0 / (hw + 1e-7)
    ndc = torch.stack([hx * pw, hy * pw], dim=1)
    if cov3D is None:
        r, qx, qy, qz = rots[:, 0], rots[:, 1], rots[:, 2], rots[:, 3]
        R = torch.stack([
            1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
            2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
            2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], dim=1).reshape(-1, 3, 3)
        L = R * (scale_mod * scales)[:, None, :]
        S = L @ L.transpose(1, 2)
    else:
        c = cov3D
        S = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]],
                        dim=1).reshape(-1, 3, 3)
    W, H = cam.width, cam.height
    fx, fy = W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy)
    limx, limy = 1.3 * cam.tanfovx, 1.3 * cam.tanfovy
    txtz, tytz = tx / tz, ty / tz
    cx = torch.clamp(txtz, -limx, limx) * tz
    cy = torch.clamp(tytz, -limy, limy) * tz
    if band_grad == "upstream":
        cx = torch.where(txtz.detach().abs() > limx, cx.detach(), tx)
        cy = torch.where(tytz.detach().abs() > limy, cy.detach(), ty)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * cx) / (tz * tz), zero, fy / tz, -(fy * cy) / (tz * tz)],
                    dim=1).reshape(-1, 2, 3)
    Wv = torch.stack([V[:, 0], V[:, 4], V[:, 8], V[:, 1], V[:, 5], V[:, 9], V[:, 2], V[:, 6], V[:, 10]],
                     dim=1).reshape(-1, 3, 3)
    T = J @ Wv
    cov = T @ S @ T.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, c2 = a0 + 0.3, c0 + 0.3
    det = a * c2 - b * b
    conic = torch.stack([c2 / det, -b / det, a / det], dim=1)
    opacity = opac.reshape(-1)
    if antialias:
        opacity = opacity * torch.sqrt(torch.clamp_min((a0 * c0 - b * b) / det, 0.000025))
    xy = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    sh_sum = None
    if colors is None:
        dv = means - cp
        dirs = dv / torch.sqrt((dv * dv).sum(1, keepdim=True))
        basis = sh_basis(D, dirs[:, 0], dirs[:, 1], dirs[:, 2])
        nb = (D + 1) ** 2
        coeffs = sh_dc.reshape(P, 1, 3) if nb == 1 else torch.cat([sh_dc.reshape(P, 1, 3), sh_rest[:, :nb - 1]], dim=1)
        sh_sum = (basis[:, :, None] * coeffs).sum(1) + 0.5
        rgb = torch.clamp_min(sh_sum, 0.0)
    else:
        rgb = colors
    return dict(xy=xy, depth=tz, conic=conic, opacity=opacity, rgb=rgb, ndc=ndc, tz=tz,
                value=1.0 / tz if inverse_depth else tz, sh_sum=sh_sum, txtz=txtz, tytz=tytz,
                limx=limx, limy=limy, V=V, Pm=Pm, campos=cp)


def camera_terms(pre) -> torch.Tensor:
    """(P, 36) per-Gaussian terms in gsr.h's dL_dcamera layout, from the expanded leaves' .grad
    (after a backward through `pre`)."""
    P = pre["V"].shape[0]
    g = lambda k, n: pre[k].grad if pre[k].grad is not None else torch.zeros((P, n), dtype=DT)
    return torch.cat([g("V", 16), g("Pm", 16), g("campos", 3), torch.zeros((P, 1), dtype=DT)], dim=1)


def terms_from_grad2d(pre, grad2d, visible, depth_mode=0) -> torch.Tensor:
    """The terms for a synthetic grad2d (P, 12): the loss is linear in the per-Gaussian quantities,
    L = sum over visible g of g2[0:2] . ndc + g2[2:5] . conic + g2[5] o' + g2[6:9] . rgb + g2[9] v."""
    g2 = t64(grad2d)
    m = torch.as_tensor(visible, dtype=DT)
    per = (g2[:, 0:2] * pre["ndc"]).sum(1) + (g2[:, 2:5] * pre["conic"]).sum(1) + g2[:, 5] * pre["opacity"] + \
        (g2[:, 6:9] * pre["rgb"]).sum(1)
    if depth_mode:
        per = per + g2[:, 9] * pre["value"]
    # culled Gaussians may hold inf / nan (tz <= 0): masked out before the sum
    torch.where(m > 0, per, torch.zeros_like(per)).sum().backward()
    t = camera_terms(pre)
    return torch.where(m[:, None] > 0, t, torch.zeros_like(t))


def margins(pre, visible) -> tuple:
    """(least |SH sum - 0| over the visible Gaussians' channels (inf without SH), least distance of
    tx/tz, ty/tz to the guard-band edges): the branches the f32 kernels and float64 must agree on."""
    m = torch.as_tensor(visible, dtype=torch.bool)
    with torch.no_grad():
        sh = float("inf") if pre["sh_sum"] is None or not m.any() else float(pre["sh_sum"][m].abs().min())
        if not m.any():
            return sh, float("inf")
        bx = (pre["txtz"][m].abs() - pre["limx"]).abs().min()
        by = (pre["tytz"][m].abs() - pre["limy"]).abs().min()
        return sh, float(torch.minimum(bx, by))


# ---------------------------------------------------------------------------------------------
# synthetic cases
# ---------------------------------------------------------------------------------------------
def posed_camera(width=96, height=64, fovx_deg=60.0):
    """A camera that is neither at the origin nor axis-aligned (train_loop.look_at_camera)."""
    import math

    from conftest import pkg
    return pkg("train_loop").look_at_camera((1.7, -0.9, -3.1), (0.3, 0.2, 0.4), math.radians(fovx_deg), width, height)


def rolled_camera(width=96, height=64, fovx_deg=60.0, roll_deg=25.0):
    """posed_camera()'s centre and target, rolled about the optical axis.  A look-at camera whose up is
    the world's y has a right vector without a y component, so posed_camera()'s viewmatrix[4] is zero
    (-9e-18); after the roll none of the nine rotation entries is (the least is 0.23 in magnitude), and
    a transposed or mis-indexed V[4k+i] moves every quantity."""
    import math

    import numpy as np

    from conftest import pkg
    c, target = np.array([1.7, -0.9, -3.1]), np.array([0.3, 0.2, 0.4])
    f = target - c
    f /= np.linalg.norm(f)
    d = np.array([0.0, 1.0, 0.0])
    y = d - f * (d @ f)
    y /= np.linalg.norm(y)
    x = np.cross(y, f)
    cr, sr = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    Rt = np.stack([cr * x + sr * y, cr * y - sr * x, f])  # world -> camera rows
    fovx = math.radians(fovx_deg)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * height / width)
    return pkg("graphics").make_camera(Rt.T, -Rt @ c, fovx, fovy, width, height)


def make_case(P, D=3, colors=False, cov3D=False, seed=0, cam=None, behind=True, band=True, edge=False):
    """P Gaussians in front of `cam` (default posed_camera()), scattered over its field of view and a
    depth range, f32 numpy inputs under "inputs" (pose_reference.preprocess's keyword arguments):
    every 10th (i % 10 == 3) lies behind the camera (culled), every 20th (i % 20 == 7) is a large
    Gaussian centred outside the 1.3 tan(fov) guard band whose footprint still reaches the image
    (xmul = 0).  SH coefficients are drawn for degree 3 and the DC term of any channel whose colour sum
    comes within 5e-3 of the clamp at 0 is moved away from it.  "grad2d": (P, 12) standard normal, slots
    10 and 11 zero.  "visible": dense_reference.geometry_f32's decision.

    edge=True (the edge scene; every extra draw is made inside this option, so the default cases are
    unchanged) adds, by index: i % 20 == 17 the same large out-of-band Gaussians in y (ymul = 0);
    i % 20 == 11 small Gaussians just inside the near plane (z in [0.21, 0.5], visible); i % 20 == 1
    small ones in front of the camera but nearer than 0.2 (z in [0.02, 0.19], culled, not by tz <= 0);
    i % 4 == 0 opacities in [0.992, 1.0], so alpha saturates at 0.99 around those centres; the behind
    class is redrawn with z in [-5, 0].  "classes": name -> boolean row mask (EDGE_CLASSES)."""
    import numpy as np
    cam = cam or posed_camera()
    rng = np.random.default_rng(1000 + seed)
    wv = np.asarray(cam.viewmatrix, np.float64).reshape(4, 4)
    i = np.arange(P)
    z = rng.uniform(2.0, 7.0, P)
    u = rng.uniform(-1.1, 1.1, (P, 2)) * np.array([cam.tanfovx, cam.tanfovy])
    log_s = rng.uniform(np.log(0.02), np.log(0.3), (P, 3))
    if band:
        far = i % 20 == 7
        u[far, 0] = rng.choice([-1.0, 1.0], int(far.sum())) * rng.uniform(1.4, 1.6, int(far.sum())) * cam.tanfovx
        z[far] = rng.uniform(3.0, 5.0, int(far.sum()))
        log_s[far] = np.log(rng.uniform(0.7, 1.0, (int(far.sum()), 3)))
    if behind:
        back = i % 10 == 3
        z[back] = rng.uniform(-5.0, 0.1, int(back.sum()))
    small = np.zeros(P, bool)
    if edge:
        n = lambda m: int(m.sum())
        back, far_y, near_in, near_out = i % 10 == 3, i % 20 == 17, i % 20 == 11, i % 20 == 1
        z[back] = rng.uniform(-5.0, 0.0, n(back))
        u[far_y, 1] = rng.choice([-1.0, 1.0], n(far_y)) * rng.uniform(1.4, 1.6, n(far_y)) * cam.tanfovy
        z[far_y] = rng.uniform(3.0, 5.0, n(far_y))
        log_s[far_y] = np.log(rng.uniform(0.7, 1.0, (n(far_y), 3)))
        z[near_in] = rng.uniform(0.21, 0.5, n(near_in))
        z[near_out] = rng.uniform(0.02, 0.19, n(near_out))
        small = near_in | near_out
        u[small] *= 0.8
        log_s[small] = np.log(rng.uniform(0.002, 0.01, (n(small), 3)))
    pv = np.stack([u[:, 0] * z, u[:, 1] * z, z], 1)
    means = (pv - wv[3, :3]) @ wv[:3, :3].T
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    inputs = dict(means=f32(means), opac=f32(rng.uniform(0.1, 0.9, P)), D=int(D))
    if edge:
        opaque = i % 4 == 0
        inputs["opac"][opaque] = f32(rng.uniform(0.992, 1.0, int(opaque.sum())))
    scales, rots = f32(np.exp(log_s)), f32(q)
    if cov3D:
        r, x, y, w = (rots[:, k].astype(np.float64) for k in range(4))
        R = np.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                      2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                      2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
        L = R * scales.astype(np.float64)[:, None, :]
        S = L @ L.transpose(0, 2, 1)
        inputs["cov3D"] = f32(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1))
    else:
        inputs["scales"], inputs["rots"] = scales, rots
    if colors:
        inputs["colors"] = f32(rng.uniform(0.0, 1.0, (P, 3)))
    else:
        inputs["sh_dc"] = f32(0.5 * rng.standard_normal((P, 1, 3)))
        inputs["sh_rest"] = f32(0.3 * rng.standard_normal((P, 15, 3)))
        for _ in range(4):  # move colour sums off the clamp
            with torch.no_grad():
                s = preprocess(cam, **inputs)["sh_sum"].numpy()
            near = np.abs(s) < 5e-3
            if not near.any():
                break
            inputs["sh_dc"][:, 0, :][near] += np.float32(0.1)
    g2 = rng.standard_normal((P, 12))
    g2[:, 10:] = 0.0
    geom = geometry_f32(cam, inputs["means"], inputs["opac"], inputs.get("scales"), inputs.get("rots"),
                        inputs.get("cov3D"))
    case = dict(cam=cam, inputs=inputs, grad2d=f32(g2), visible=geom["visible"].numpy().copy(), geom=geom)
    if edge:
        case["classes"] = dict(band_x=i % 20 == 7, band_y=far_y, behind=back, near_in=near_in, near_out=near_out,
                               opaque=opaque)
        case["classes"]["plain"] = ~np.logical_or.reduce(list(case["classes"].values()))
    return case


EDGE_VISIBLE = ("band_x", "band_y", "near_in", "opaque", "plain")  # the classes whose members are (mostly) visible
EDGE_CULLED = ("behind", "near_out")                               # entirely culled
