"""Camera pose refinement on top of the rasterizer's camera gradients (gsr.h gsr_backward_posed).

The kernels return dL/dviewmatrix, dL/dprojmatrix and dL/dcampos with the three camera fields treated
as independent inputs.  This module ties them to one rigid correction per view and chains the 36
numbers to its six parameters, in float64 on the host (a 4 x 4 product and an inverse: nothing a
device helps with).

Parametrisation: delta = (omega, tau) in R^6 acts in the CAMERA frame, in the repository's row-vector
convention (graphics.py: p_view = p_world @ world_view[:3, :3] + world_view[3, :3]):

    world_view' = world_view @ D(delta),   D[:3, :3] = Exp(omega)^T,   D[3, :3] = tau

i.e. p_view' = Exp(omega) p_view + tau: omega is an axis-angle rotation of the camera's view space
(radians), tau a translation of it (scene units).  delta = 0 is the camera itself.

``compose`` keeps the camera's own rounding: each field is the stored f32 value plus the change the
correction makes, evaluated in float64 -- full_proj' = full_proj + (world_view' - world_view) @ proj with
proj = graphics.get_projection_matrix(znear, zfar, fovx, fovy)^T, campos' = campos + (centre' - centre)
with centre = inv(world_view)[3, :3] -- so compose(cam, 0) is cam bit for bit (the fields of a camera
were rounded to f32 from float64 products this module cannot redo from the f32 values), and for any
delta the fields differ from world_view' @ proj and inv(world_view')[3, :3] by that same f32 rounding.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import graphics
from .graphics import RasterCamera

SERIES_BELOW = 1e-3  # |omega| under which Exp uses its power series (sin t / t, (1 - cos t) / t^2)


def _skew(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def so3_exp(omega: torch.Tensor, series: bool | None = None) -> torch.Tensor:
    """Exp(omega) = I + a K + b K^2, K = [omega]x, a = sin t / t, b = (1 - cos t) / t^2 (Rodrigues); for
    t = |omega| < SERIES_BELOW the coefficients' series in t^2, which is differentiable at 0.
    `series` forces a branch (tests)."""
    omega = torch.as_tensor(omega, dtype=torch.float64)
    t2 = (omega * omega).sum()
    if series is None:
        series = float(t2.detach()) < SERIES_BELOW * SERIES_BELOW
    if series:
        a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0
        b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        t = torch.sqrt(t2)
        a = torch.sin(t) / t
        h = torch.sin(0.5 * t)
        b = 2.0 * h * h / t2  # 1 - cos t without the cancellation
    K = _skew(omega)
    return torch.eye(3, dtype=torch.float64) + a * K + b * (K @ K)


def delta_matrix(delta, series: bool | None = None) -> torch.Tensor:
    """D(delta), 4 x 4 float64, differentiable in delta (6,)."""
    delta = torch.as_tensor(delta, dtype=torch.float64).reshape(6)
    R = so3_exp(delta[:3], series)
    top = torch.cat([R.transpose(0, 1), torch.zeros((3, 1), dtype=torch.float64)], dim=1)
    bottom = torch.cat([delta[3:], torch.ones(1, dtype=torch.float64)])[None]
    return torch.cat([top, bottom], dim=0)


def _fields(cam: RasterCamera, delta: torch.Tensor):
    """(viewmatrix (16,), projmatrix (16,), campos (3,)) of the corrected camera as float64 tensors,
    differentiable in delta."""
    wv = torch.as_tensor(np.asarray(cam.viewmatrix, np.float64).reshape(4, 4))
    full = torch.as_tensor(np.asarray(cam.projmatrix, np.float64).reshape(4, 4))
    centre = torch.as_tensor(np.asarray(cam.campos, np.float64).reshape(3))
    fovx, fovy = 2.0 * math.atan(cam.tanfovx), 2.0 * math.atan(cam.tanfovy)
    proj = torch.as_tensor(graphics.get_projection_matrix(cam.znear, cam.zfar, fovx, fovy).T.copy())
    wv2 = wv @ delta_matrix(delta)
    full2 = full + (wv2 - wv) @ proj
    centre2 = centre + (torch.linalg.inv(wv2)[3, :3] - torch.linalg.inv(wv)[3, :3])
    return wv2.reshape(16), full2.reshape(16), centre2


def compose(cam: RasterCamera, delta) -> RasterCamera:
    """The camera `cam` corrected by delta: float64 on the host, cast to f32 at the boundary like
    graphics.make_camera.  Size, field of view and clip planes are cam's."""
    with torch.no_grad():
        v, p, c = _fields(cam, torch.as_tensor(delta, dtype=torch.float64).detach().reshape(6))
    f32 = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float32)
    return dataclasses.replace(cam, viewmatrix=f32(v), projmatrix=f32(p), campos=f32(c))


def chain(cam: RasterCamera, delta, dL_dcamera) -> torch.Tensor:
    """dL/ddelta (6,) float64 from the kernels' 36 floats (viewmatrix[16], projmatrix[16], campos[3], 0),
    by float64 autograd through the composition."""
    g = torch.as_tensor(dL_dcamera).detach().to("cpu", torch.float64).reshape(-1)
    with torch.enable_grad():  # also inside an autograd Function's backward, which runs without grad mode
        d = torch.as_tensor(delta, dtype=torch.float64).detach().reshape(6).clone().requires_grad_(True)
        v, p, c = _fields(cam, d)
        L = (v * g[0:16]).sum() + (p * g[16:32]).sum() + (c * g[32:35]).sum()
        return torch.autograd.grad(L, d)[0]


def pose_error(cam_a: RasterCamera, cam_b: RasterCamera) -> tuple:
    """(angle in radians of the rotation between the two cameras, distance between their centres)."""
    Ra = np.asarray(cam_a.viewmatrix, np.float64).reshape(4, 4)[:3, :3]
    Rb = np.asarray(cam_b.viewmatrix, np.float64).reshape(4, 4)[:3, :3]
    M = Ra.T @ Rb
    # atan2 of the skew part's norm and the trace: accurate near 0 where acos is not
    s = 0.5 * math.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2)
    c = 0.5 * (np.trace(M) - 1.0)
    dist = float(np.linalg.norm(np.asarray(cam_a.campos, np.float64) - np.asarray(cam_b.campos, np.float64)))
    return float(math.atan2(s, c)), dist
