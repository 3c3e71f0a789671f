"""Python mirror of the rasterizer surface.

Two entry points, both ending in the same HIP kernels:

* ``CAbiRasterizer`` -- drives the C ABI (include/gsr/gsr.h) through ctypes with torch-owned
  device memory: what a ctypes / cgo / JNI binding of libgsr_hip.so looks like.  The GPU parity
  tests and bench.py use it so every call crosses the C boundary.
* ``render()`` / ``rasterize_gaussians()`` -- the libtorch RasterizeGaussians autograd Function
  (lib/_gsr_torch*.so), i.e. the C++ render() surface (csrc/torch/gsr_render.h) the
  reference's training loop would call at src/utils/train_utils.cpp:137-144.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import native
from .graphics import RasterCamera

INT32_MAX = 2**31 - 1
# gsr.h gsr_scores, in the struct's order (hits is uint32 there; torch has no arithmetic on it)
SCORE_NAMES = ("max_w", "sum_w", "hits")
SCORE_DTYPES = {"max_w": torch.float32, "sum_w": torch.float32, "hits": torch.int32}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _f32(t, shape=None, device=None):
    if t is None:
        return None
    t = torch.as_tensor(t, dtype=torch.float32, device=device)
    if shape is not None:
        t = t.reshape(shape)
    return t.contiguous()


class _Allocator:
    """Allocation callbacks for the C ABI: uint8 tensors kept alive by the owner.  With `reuse`
    (a list kept by the caller across calls), the i-th request of a call gets the i-th tensor
    of the previous call when it is large enough -- a step loop then allocates nothing (the
    previous step's buffers are dead by the time the next step's kernels run: one stream)."""

    def __init__(self, device, reuse: list | None = None):
        self.device = device
        self.tensors = []
        self.reuse = reuse
        self.cb = native.ALLOC_FN(self._alloc)

    def _alloc(self, _ctx, nbytes):
        n = max(int(nbytes), 16)
        i = len(self.tensors)
        if self.reuse is not None and i < len(self.reuse) and self.reuse[i].numel() >= n:
            t = self.reuse[i]
        else:
            t = torch.empty(n, dtype=torch.uint8, device=self.device)
            if self.reuse is not None:
                if i < len(self.reuse):
                    self.reuse[i] = t
                else:
                    self.reuse.append(t)
        self.tensors.append(t)
        return t.data_ptr()


class _CallState:
    """What a forward's state object can ask the library afterwards.  The subclass names the camera
    struct and the entry count the library was called with: `_call_camera()`, `_call_entries()`."""

    @property
    def num_rendered(self) -> int:
        """K.  Under a binning bound (max_rendered > 0) K stays on the device until asked for:
        the first access reads it back (synchronising the stream) and raises on an overflow."""
        if self.buffers.num_rendered < 0:
            k = ctypes.c_int32(0)
            rc = native.load_hip().gsr_read_num_rendered(
                ctypes.byref(self._call_camera()), ctypes.byref(self.buffers), ctypes.byref(k),
                ctypes.c_void_p(torch.cuda.current_stream(self.color.device).cuda_stream))
            if rc == native.GSR_ERR_OVERFLOW:
                raise OverflowError(native.last_error())
            if rc != 0:
                raise RuntimeError(f"gsr_read_num_rendered failed ({rc}): {native.last_error()}")
            self.buffers.num_rendered = k.value
        return int(self.buffers.num_rendered)

    def _owner(self, ptr: int):
        for a in self.allocs:
            for t in a.tensors:
                base = t.data_ptr()
                if base <= ptr < base + t.numel():
                    return t, ptr - base
        raise KeyError("pointer not inside a forward buffer")

    def _view_ptr(self, what: int):
        return native.load_hip().gsr_view(ctypes.byref(self._call_camera()), self._call_entries(),
                                          ctypes.byref(self.buffers), what)

    def view(self, what: int, dtype: torch.dtype, count: int) -> torch.Tensor:
        """Copy of an internal array (gsr_view) as a torch tensor."""
        p = self._view_ptr(what)
        if not p or count == 0:
            return torch.empty(0, dtype=dtype, device=self.color.device)
        t, off = self._owner(p)
        nbytes = count * torch.empty(0, dtype=dtype).element_size()
        return t[off:off + nbytes].view(dtype).clone()


@dataclass
class ForwardState(_CallState):
    cam: RasterCamera
    inputs: dict
    settings: native.Settings
    gauss: native.Gaussians
    buffers: native.Buffers
    color: torch.Tensor
    radii: torch.Tensor
    allocs: list = field(default_factory=list)
    depth: torch.Tensor | None = None   # forward_aux: (H, W) sum w v (v = z, or 1 / z)
    alpha: torch.Tensor | None = None   # forward_aux: (H, W) sum w = 1 - final T

    def _call_camera(self):
        return native.camera_struct(self.cam)

    def _call_entries(self) -> int:
        return self.gauss.P

    def k_device(self) -> torch.Tensor:
        """K as a 1-element int32 device tensor aliasing the scan's counter (no copy, no sync)."""
        p = self._view_ptr(native.VIEW_COUNTS)
        if not p:
            raise RuntimeError("gsr_view(COUNTS) returned NULL")
        t, off = self._owner(p)
        return t[off:off + 4].view(torch.int32)


@dataclass
class ViewsState(_CallState):
    """gsr_forward_views' outputs, kept for gsr_backward_views (one set of buffers for all views).
    num_rendered is K over all views; view() sees the tall grid and the V * P (view, Gaussian)
    entries e = v * P + g: sorted tiles are tall-grid tile ids, sorted gids are entry ids."""
    cams: list
    cstructs: object          # the gsr_camera array handed to the library
    inputs: dict
    settings: native.Settings
    gauss: native.Gaussians
    buffers: native.Buffers
    color: torch.Tensor       # V x 3 x H x W
    radii: torch.Tensor       # V x P
    allocs: list

    def tall_camera(self):
        """The pass's camera struct: the views stacked as bands of ceil(H / 16) tile rows."""
        tall = native.Camera()
        ctypes.memmove(ctypes.byref(tall), ctypes.byref(self.cstructs[0]), ctypes.sizeof(tall))
        tall.height = len(self.cams) * ((self.cams[0].height + 15) // 16) * 16
        return tall

    _call_camera = tall_camera

    def _call_entries(self) -> int:
        return len(self.cams) * self.gauss.P


class CAbiRasterizer:
    """Thin ctypes front-end of gsr_forward / gsr_backward*."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.L = native.load_hip()
        self._cams = {}  # camera contents -> gsr_camera struct

    @staticmethod
    def _cam_key(cam):
        """Everything camera_struct reads, by value: an in-place edit of a camera's matrices or
        size gives a new key, never a stale struct (a stale width / height would size the
        kernels' writes differently from the colour tensor made from the new camera)."""
        return (int(cam.width), int(cam.height), float(cam.tanfovx), float(cam.tanfovy),
                np.asarray(cam.viewmatrix, np.float32).tobytes(), np.asarray(cam.projmatrix, np.float32).tobytes(),
                np.asarray(cam.campos, np.float32).tobytes())

    def _cam(self, cam):
        key = self._cam_key(cam)
        c = self._cams.get(key)
        if c is not None:
            return c
        c = native.camera_struct(cam)
        if len(self._cams) > 256:
            self._cams.clear()
        self._cams[key] = c
        return c

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {native.last_error()}")

    def _prepare(self, means3D, opacities, scales, rotations, sh_dc, sh_rest, sh_degree, colors_precomp,
                 cov3D_precomp, scale_modifier, bg, tile_rows, max_rendered, debug, antialiasing=False):
        dev = self.device
        means3D = _f32(means3D, device=dev)
        P = int(means3D.shape[0])
        inputs = dict(means3D=means3D.reshape(P, 3), opacities=_f32(opacities, (P,), dev),
                      scales=_f32(scales, (P, 3), dev) if scales is not None else None,
                      rotations=_f32(rotations, (P, 4), dev) if rotations is not None else None,
                      sh_dc=_f32(sh_dc, (P, 1, 3), dev) if sh_dc is not None else None,
                      sh_rest=_f32(sh_rest, device=dev) if sh_rest is not None else None,
                      colors_precomp=_f32(colors_precomp, (P, 3), dev) if colors_precomp is not None else None,
                      cov3D_precomp=_f32(cov3D_precomp, (P, 6), dev) if cov3D_precomp is not None else None)
        if inputs["sh_rest"] is not None:
            inputs["sh_rest"] = inputs["sh_rest"].reshape(P, -1, 3).contiguous()
            if inputs["sh_rest"].shape[1] == 0:
                inputs["sh_rest"] = None
        g = native.Gaussians()
        g.P, g.sh_degree, g.scale_modifier = P, int(sh_degree), float(scale_modifier)
        g.sh_rest_coeffs = 0 if inputs["sh_rest"] is None else int(inputs["sh_rest"].shape[1])
        for k in ("means3D", "sh_dc", "sh_rest", "colors_precomp", "opacities", "scales", "rotations",
                  "cov3D_precomp"):
            setattr(g, k, None if inputs[k] is None else inputs[k].data_ptr())
        s = native.Settings()
        s.bg[:] = [float(v) for v in bg]
        s.tile_y0, s.tile_y1 = (0, INT32_MAX) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        # the state keeps these settings, so every backward passes the forward's flags
        s.flags = (native.GSR_FLAG_DEBUG if debug else 0) | (native.GSR_FLAG_ANTIALIAS if antialiasing else 0)
        s.max_rendered = int(max_rendered)
        return inputs, g, s

    def _forward(self, cam: RasterCamera, inverse_depth, *prep) -> ForwardState:
        """gsr_forward, or gsr_forward_aux when inverse_depth is not None; prep: _prepare's arguments."""
        dev = self.device
        inputs, g, s = self._prepare(*prep)
        P, H, W = g.P, cam.height, cam.width
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        ag, ab, ai = _Allocator(dev), _Allocator(dev), _Allocator(dev)
        bufs = native.Buffers()
        args = (ctypes.byref(self._cam(cam)), ctypes.byref(g), ctypes.byref(s), _ptr(color),
                _ptr(radii) if P else None, ag.cb, ab.cb, ai.cb, None, ctypes.byref(bufs), self._stream())
        depth = alpha = None
        if inverse_depth is None:
            self._check(self.L.gsr_forward(*args), "gsr_forward")
        else:
            s.flags |= native.GSR_FLAG_AUX | (native.GSR_FLAG_INVDEPTH if inverse_depth else 0)
            depth = torch.empty((H, W), dtype=torch.float32, device=dev)
            alpha = torch.empty((H, W), dtype=torch.float32, device=dev)
            aux = native.AuxOut(depth.data_ptr(), alpha.data_ptr())
            self._check(self.L.gsr_forward_aux(*args, ctypes.byref(aux)), "gsr_forward_aux")
        return ForwardState(cam=cam, inputs=inputs, settings=s, gauss=g, buffers=bufs, color=color,
                            radii=radii, allocs=[ag, ab, ai], depth=depth, alpha=alpha)

    def forward(self, cam: RasterCamera, means3D, opacities, scales=None, rotations=None, sh_dc=None,
                sh_rest=None, sh_degree=0, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0,
                bg=(0.0, 0.0, 0.0), tile_rows=None, max_rendered=0, debug=False,
                antialiasing=False) -> ForwardState:
        """gsr_forward.  max_rendered > 0 sizes the binning for that many instances and skips the
        host read of K (see ForwardState.num_rendered).  antialiasing: GSR_FLAG_ANTIALIAS, the
        opacity compensation for the 0.3 px^2 dilation; the returned state carries it to backward()."""
        return self._forward(cam, None, means3D, opacities, scales, rotations, sh_dc, sh_rest, sh_degree,
                             colors_precomp, cov3D_precomp, scale_modifier, bg, tile_rows, max_rendered, debug,
                             antialiasing)

    def forward_aux(self, cam: RasterCamera, means3D, opacities, scales=None, rotations=None, sh_dc=None,
                    sh_rest=None, sh_degree=0, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0,
                    bg=(0.0, 0.0, 0.0), tile_rows=None, max_rendered=0, debug=False,
                    inverse_depth=False, antialiasing=False) -> ForwardState:
        """gsr_forward_aux: forward() plus .depth = sum w z (sum w / z with inverse_depth) and
        .alpha = sum w per pixel, over the pairs the colour pass blends.  Full images only."""
        return self._forward(cam, bool(inverse_depth), means3D, opacities, scales, rotations, sh_dc, sh_rest,
                             sh_degree, colors_precomp, cov3D_precomp, scale_modifier, bg, tile_rows, max_rendered,
                             debug, antialiasing)

    def _backward(self, st: ForwardState, dL_dpix, aux_grads=None, camera_grad=False) -> dict:
        """gsr_backward, or gsr_backward_aux with aux_grads = (dL_ddepth, dL_dalpha), each None = zero;
        camera_grad: gsr_backward_posed, the same call followed by the camera pass."""
        H, W = st.cam.height, st.cam.width
        dpix = _f32(dL_dpix, (3, H, W), self.device)
        out, gg = self._grad_tensors(st)
        scratch = _Allocator(self.device)
        args = (ctypes.byref(self._cam(st.cam)), ctypes.byref(st.gauss), ctypes.byref(st.settings),
                ctypes.byref(st.buffers), _ptr(dpix), scratch.cb, None, ctypes.byref(gg), self._stream())
        aux = None
        if aux_grads is not None:
            dd, da = (_f32(t, (H, W), self.device) for t in aux_grads)
            aux = native.AuxGrads(None if dd is None else dd.data_ptr(), None if da is None else da.data_ptr())
        if camera_grad:
            dcam = torch.empty(native.CAMERA_GRAD_FLOATS, dtype=torch.float32, device=self.device)
            rc = self.L.gsr_backward_posed(*args[:5], None if aux is None else ctypes.byref(aux), scratch.cb, None,
                                           ctypes.byref(gg), _ptr(dcam), self._stream())
            self._check(rc, "gsr_backward_posed")
            out.update(self._camera_views(dcam))
        elif aux is None:
            self._check(self.L.gsr_backward(*args), "gsr_backward")
        else:
            self._check(self.L.gsr_backward_aux(*args, ctypes.byref(aux)), "gsr_backward_aux")
        return out

    @staticmethod
    def _camera_views(dcam: torch.Tensor) -> dict:
        """The 36 floats of gsr.h's dL_dcamera ("camera") and its three fields as views of it,
        flattened like RasterCamera's."""
        return dict(camera=dcam, viewmatrix=dcam[0:16], projmatrix=dcam[16:32], campos=dcam[32:35])

    def backward(self, st: ForwardState, dL_dpix, camera_grad=False) -> dict:
        """gsr_backward.  camera_grad: gsr_backward_posed -- the same leaf gradients bit for bit, and
        the dict gains "viewmatrix" (16,), "projmatrix" (16,), "campos" (3,): dL/d(the camera's field),
        the three treated as independent (pose.chain ties them to a pose), device views of the
        36-float "camera".  Full images only."""
        return self._backward(st, dL_dpix, None, camera_grad)

    def backward_aux(self, st: ForwardState, dL_dpix, dL_ddepth=None, dL_dalpha=None, camera_grad=False) -> dict:
        """gsr_backward_aux: backward() for a loss over colour, depth and alpha (None = zero).
        camera_grad: as backward()'s; the depth channel's dependence on the view matrix is included."""
        return self._backward(st, dL_dpix, (dL_ddepth, dL_dalpha), camera_grad)

    def backward_camera(self, st: ForwardState, grad2d: torch.Tensor, depth_mode: int = 0) -> dict:
        """gsr_backward_camera: the camera pass alone on a (P, 12) grad2d (backward_blend's; depth_mode
        1 / 2 read slot 9 as dL/dz / dL/d(1/z) of the depth channel).  The camera keys of backward()."""
        grad2d = grad2d.contiguous()
        nbytes = int(self.L.gsr_camera_grad_scratch_bytes(st.gauss.P))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        dcam = torch.empty(native.CAMERA_GRAD_FLOATS, dtype=torch.float32, device=self.device)
        c = self._cam(st.cam)
        rc = self.L.gsr_backward_camera(ctypes.byref(c), ctypes.byref(st.gauss), ctypes.byref(st.settings),
                                        ctypes.byref(st.buffers), _ptr(grad2d), int(depth_mode), _ptr(scratch),
                                        _ptr(dcam), self._stream())
        self._check(rc, "gsr_backward_camera")
        return self._camera_views(dcam)

    def forward_batch(self, cams, means3D, opacities, scales=None, rotations=None, sh_dc=None, sh_rest=None,
                      sh_degree=0, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0,
                      bg=(0.0, 0.0, 0.0), max_rendered=0, debug=False, antialiasing=False) -> list:
        """gsr_forward_batch: one ForwardState per camera (full images), one host wait in total
        (none with max_rendered > 0)."""
        dev = self.device
        inputs, g, s = self._prepare(means3D, opacities, scales, rotations, sh_dc, sh_rest, sh_degree,
                                     colors_precomp, cov3D_precomp, scale_modifier, bg, None, max_rendered, debug,
                                     antialiasing)
        V, P = len(cams), g.P
        colors = [torch.empty((3, c.height, c.width), dtype=torch.float32, device=dev) for c in cams]
        radii = [torch.empty((P,), dtype=torch.int32, device=dev) for _ in cams]
        ag, ab, ai = _Allocator(dev), _Allocator(dev), _Allocator(dev)
        bufs = (native.Buffers * V)()
        cs = (native.Camera * V)(*[native.camera_struct(c) for c in cams])
        col_p = (ctypes.c_void_p * V)(*[t.data_ptr() for t in colors])
        rad_p = (ctypes.c_void_p * V)(*[t.data_ptr() for t in radii])
        rc = self.L.gsr_forward_batch(V, cs, ctypes.byref(g), ctypes.byref(s), col_p, rad_p if P else None, ag.cb,
                                      ab.cb, ai.cb, None, bufs, self._stream())
        self._check(rc, "gsr_forward_batch")
        out = []
        for v, cam in enumerate(cams):
            b = native.Buffers()
            ctypes.memmove(ctypes.byref(b), ctypes.byref(bufs[v]), ctypes.sizeof(b))
            out.append(ForwardState(cam=cam, inputs=inputs, settings=s, gauss=g, buffers=b, color=colors[v],
                                    radii=radii[v], allocs=[ag, ab, ai]))
        return out

    def forward_views(self, cams, means3D, opacities, scales=None, rotations=None, sh_dc=None, sh_rest=None,
                      sh_degree=0, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0,
                      bg=(0.0, 0.0, 0.0), max_rendered=0, debug=False, antialiasing=False) -> "ViewsState":
        """gsr_forward_views: V same-size cameras in one pass (one launch per stage).  color is
        V x 3 x H x W, radii V x P; bit-identical to V forward() calls."""
        dev = self.device
        inputs, g, s = self._prepare(means3D, opacities, scales, rotations, sh_dc, sh_rest, sh_degree,
                                     colors_precomp, cov3D_precomp, scale_modifier, bg, None, max_rendered, debug,
                                     antialiasing)
        V, P = len(cams), g.P
        H, W = cams[0].height, cams[0].width
        color = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((V, P), dtype=torch.int32, device=dev)
        ag, ab, ai = _Allocator(dev), _Allocator(dev), _Allocator(dev)
        bufs = native.Buffers()
        cs = (native.Camera * V)(*[self._cam(c) for c in cams])
        rc = self.L.gsr_forward_views(V, cs, ctypes.byref(g), ctypes.byref(s), _ptr(color),
                                      _ptr(radii) if P else None, ag.cb, ab.cb, ai.cb, None, ctypes.byref(bufs),
                                      self._stream())
        self._check(rc, "gsr_forward_views")
        return ViewsState(cams=list(cams), cstructs=cs, inputs=inputs, settings=s, gauss=g, buffers=bufs,
                          color=color, radii=radii, allocs=[ag, ab, ai])

    def backward_views(self, st: "ViewsState", dL_dpix) -> dict:
        """gsr_backward_views: means2D / conic gradients per view (V x P x 3), leaf gradients
        summed over the views in view order."""
        V = len(st.cams)
        dpix = _f32(dL_dpix, (V, 3, st.cams[0].height, st.cams[0].width), self.device)
        out, gg = self._grad_tensors(st)
        P = st.gauss.P
        for k, name in (("means2D", "dL_dmeans2D"), ("conic", "dL_dconic")):
            out[k] = torch.empty((V, P, 3), dtype=torch.float32, device=self.device)
            setattr(gg, name, out[k].data_ptr())
        scratch = _Allocator(self.device)
        rc = self.L.gsr_backward_views(V, st.cstructs, ctypes.byref(st.gauss), ctypes.byref(st.settings),
                                       ctypes.byref(st.buffers), _ptr(dpix), scratch.cb, None, ctypes.byref(gg),
                                       self._stream())
        self._check(rc, "gsr_backward_views")
        return out

    def _grad_tensors(self, st: ForwardState, P: int | None = None):
        P = st.gauss.P if P is None else P
        dev = self.device
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = dict(means2D=e(P, 3), conic=e(P, 3), opacities=e(P, 1), means3D=e(P, 3))
        inp = st.inputs
        if inp["colors_precomp"] is not None:
            out["colors"] = e(P, 3)
        else:
            out["sh_dc"] = e(P, 1, 3)
            if inp["sh_rest"] is not None:
                out["sh_rest"] = inp["sh_rest"].new_empty((P,) + tuple(inp["sh_rest"].shape[1:]))
        if inp["cov3D_precomp"] is not None:
            out["cov3D"] = e(P, 6)
        else:
            out["scales"], out["rotations"] = e(P, 3), e(P, 4)
        gg = native.Grads()
        names = dict(means2D="dL_dmeans2D", conic="dL_dconic", opacities="dL_dopacity", colors="dL_dcolors",
                     means3D="dL_dmeans3D", sh_dc="dL_dsh_dc", sh_rest="dL_dsh_rest", scales="dL_dscales",
                     rotations="dL_drotations", cov3D="dL_dcov3D")
        for k, v in out.items():
            setattr(gg, names[k], v.data_ptr())
        return out, gg

    def backward_blend(self, st: ForwardState, dL_dpix, out: torch.Tensor | None = None) -> torch.Tensor:
        """B1 + per-Gaussian sum -> grad2d (P x 12).  `out`: optional contiguous (>= P) x 12
        tensor to write into."""
        dpix = _f32(dL_dpix, (3, st.cam.height, st.cam.width), self.device)
        if out is None:
            grad2d = torch.empty((st.gauss.P, native.GSR_GRAD2D_STRIDE), dtype=torch.float32, device=self.device)
        else:
            if not (out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] >= st.gauss.P
                    and out.shape[1] == native.GSR_GRAD2D_STRIDE):
                raise ValueError("backward_blend: out must be a contiguous f32 (>= P) x 12 tensor")
            grad2d = out
        scratch = _Allocator(self.device)
        c = self._cam(st.cam)
        rc = self.L.gsr_backward_blend(ctypes.byref(c), ctypes.byref(st.gauss), ctypes.byref(st.settings),
                                       ctypes.byref(st.buffers), _ptr(dpix), scratch.cb, None, _ptr(grad2d),
                                       self._stream())
        self._check(rc, "gsr_backward_blend")
        return grad2d

    def backward_preprocess(self, st: ForwardState, grad2d: torch.Tensor) -> dict:
        out, gg = self._grad_tensors(st)
        grad2d = grad2d.contiguous()
        c = self._cam(st.cam)
        rc = self.L.gsr_backward_preprocess(ctypes.byref(c), ctypes.byref(st.gauss), ctypes.byref(st.settings),
                                            ctypes.byref(st.buffers), _ptr(grad2d), ctypes.byref(gg),
                                            self._stream())
        self._check(rc, "gsr_backward_preprocess")
        return out

    def scores(self, st: ForwardState, into: dict | None = None) -> dict:
        """gsr_forward_scores on a forward's state (forward / forward_aux / one of forward_batch's):
        per Gaussian, over the pixels the view blended it into with weight w = T alpha, "max_w" and
        "sum_w" (float32 (P,)) and "hits", the number of those pixels (int32 (P,)); zeros for a
        Gaussian the view does not use.  into: a dict of some or all of those tensors to combine the
        view with instead (max, +, +; accumulate = 1) -- a key left out is not computed.  Returns the
        dict written."""
        P = st.gauss.P
        if into is None:
            out = {k: torch.empty(P, dtype=SCORE_DTYPES[k], device=self.device) for k in SCORE_NAMES}
        else:
            out = into
            if not out or any(k not in SCORE_NAMES for k in out):
                raise ValueError(f"scores: into must hold some of {SCORE_NAMES}, not {sorted(out)}")
            for k, t in out.items():
                if not (t.is_contiguous() and t.dtype == SCORE_DTYPES[k] and tuple(t.shape) == (P,)
                        and t.device == st.color.device):
                    raise ValueError(f"scores: into[{k!r}] must be a contiguous {SCORE_DTYPES[k]} ({P},) tensor on "
                                     f"{st.color.device}")
        sc = native.Scores(*[out[k].data_ptr() if k in out else None for k in SCORE_NAMES])
        scratch = _Allocator(self.device)
        rc = self.L.gsr_forward_scores(ctypes.byref(self._cam(st.cam)), ctypes.byref(st.gauss),
                                       ctypes.byref(st.settings), ctypes.byref(st.buffers), scratch.cb, None,
                                       ctypes.byref(sc), 0 if into is None else 1, self._stream())
        self._check(rc, "gsr_forward_scores")
        return out


# ------------------------------------------------------------------------------------------
# multi-GPU split (gsr_shard_* / gsr_band_*): the compute of one rank
# ------------------------------------------------------------------------------------------
@dataclass
class ShardState:
    """gsr_shard_forward's outputs a rank keeps until gsr_shard_backward."""
    cam: RasterCamera
    inputs: dict
    settings: native.Settings
    gauss: native.Gaussians
    band_rows: list
    pair_cap: int
    send: torch.Tensor        # nbands exchange blocks (uint8)
    state: torch.Tensor       # gsr_shard_state_bytes (uint8)
    radii: torch.Tensor

    @property
    def counts(self) -> torch.Tensor:
        """Splats packed per band (device u32 headers; > pair_cap = overflow)."""
        nb = len(self.band_rows) - 1
        blk = self.send.numel() // nb
        return self.send.view(nb, blk).view(torch.int32)[:, 0]  # strided view of the headers


class ShardRasterizer(CAbiRasterizer):
    """The per-rank calls of the multi-GPU path; the caller moves the exchange blocks."""

    def block_bytes(self, pair_cap: int) -> int:
        return int(self.L.gsr_exchange_block_bytes(int(pair_cap)))

    def shard_forward(self, cam: RasterCamera, band_rows, pair_cap: int, means3D, opacities, scales=None,
                      rotations=None, sh_dc=None, sh_rest=None, sh_degree=0, colors_precomp=None,
                      cov3D_precomp=None, scale_modifier=1.0, row_hist: torch.Tensor | None = None,
                      debug=False, reuse: dict | None = None, row_spans: bool = False) -> ShardState:
        """`reuse` (a dict the caller keeps across steps): the send / state / radii buffers and the
        prepared input structs of the previous call with the same sizes are used again.
        row_hist (zeroed by the caller) += the instances per tile row; with row_spans it holds
        3 x grid_y u32: that, then the rect start rows and end rows (GSR_FLAG_ROW_SPANS)."""
        dev = self.device
        srcs = (means3D, opacities, scales, rotations, sh_dc, sh_rest, colors_precomp, cov3D_precomp)
        key = None
        if all(t is None or (torch.is_tensor(t) and t.is_contiguous() and t.dtype == torch.float32
                             and t.device == dev) for t in srcs):
            key = tuple(None if t is None else (t.data_ptr(), tuple(t.shape)) for t in srcs) + \
                (int(sh_degree), float(scale_modifier), bool(debug))
        if reuse is not None and key is not None and reuse.get("key") == key:
            inputs, g, s = reuse["prep"]
        else:
            inputs, g, s = self._prepare(means3D, opacities, scales, rotations, sh_dc, sh_rest, sh_degree,
                                         colors_precomp, cov3D_precomp, scale_modifier, (0.0, 0.0, 0.0), None, 0,
                                         debug)
            if reuse is not None:
                reuse["key"], reuse["prep"] = key, (inputs, g, s)
        nb = len(band_rows) - 1
        rows = (ctypes.c_int32 * (nb + 1))(*[int(r) for r in band_rows])
        nsend = nb * self.block_bytes(pair_cap)
        nstate = int(self.L.gsr_shard_state_bytes(g.P, nb, int(pair_cap)))
        if reuse is not None and reuse.get("sizes") == (nsend, nstate, g.P):
            send, state, radii = reuse["bufs"]
        else:
            send = torch.empty(nsend, dtype=torch.uint8, device=dev)
            state = torch.empty(nstate, dtype=torch.uint8, device=dev)
            radii = torch.empty((g.P,), dtype=torch.int32, device=dev)
            if reuse is not None:
                reuse["sizes"], reuse["bufs"] = (nsend, nstate, g.P), (send, state, radii)
        c = self._cam(cam)
        s.flags = (native.GSR_FLAG_DEBUG if debug else 0) | (native.GSR_FLAG_ROW_SPANS if row_spans else 0)
        if row_spans and (row_hist is None or row_hist.numel() < 3 * ((cam.height + 15) // 16)):
            raise ValueError("row_spans needs a row_hist of 3 x grid_y words")
        rc = self.L.gsr_shard_forward(ctypes.byref(c), ctypes.byref(g), ctypes.byref(s), nb, rows, int(pair_cap),
                                      _ptr(send), _ptr(radii) if g.P else None, _ptr(state), _ptr(row_hist),
                                      self._stream())
        self._check(rc, "gsr_shard_forward")
        return ShardState(cam=cam, inputs=inputs, settings=s, gauss=g, band_rows=list(band_rows),
                          pair_cap=int(pair_cap), send=send, state=state, radii=radii)

    def band_forward(self, cam: RasterCamera, tile_rows, nsrc: int, pair_cap: int, recv: torch.Tensor,
                     max_rendered: int, out_color: torch.Tensor | None = None, bg=(0.0, 0.0, 0.0),
                     debug=False, reuse: dict | None = None) -> ForwardState:
        """F2..F6 over the splats received from nsrc shards; only the band's pixels of
        out_color are written.  `reuse`: the caller's dict of buffers kept across steps."""
        dev = self.device
        s = native.Settings()
        s.bg[:] = [float(v) for v in bg]
        s.tile_y0, s.tile_y1 = int(tile_rows[0]), int(tile_rows[1])
        s.flags = native.GSR_FLAG_DEBUG if debug else 0
        s.max_rendered = int(max_rendered)
        if out_color is not None:
            color = out_color
        elif reuse is not None and "color" in reuse and tuple(reuse["color"].shape) == (3, cam.height, cam.width):
            color = reuse["color"]  # the band's pixels are rewritten; the rest stay as they were
        else:
            color = torch.zeros((3, cam.height, cam.width), dtype=torch.float32, device=dev)
            if reuse is not None:
                reuse["color"] = color
        r = (lambda k: reuse.setdefault(k, [])) if reuse is not None else (lambda k: None)
        ag, ab, ai = _Allocator(dev, r("geom")), _Allocator(dev, r("bin")), _Allocator(dev, r("img"))
        bufs = native.Buffers()
        c = self._cam(cam)
        rc = self.L.gsr_band_forward(ctypes.byref(c), ctypes.byref(s), int(nsrc), int(pair_cap), _ptr(recv),
                                     _ptr(color), ag.cb, ab.cb, ai.cb, None, ctypes.byref(bufs), self._stream())
        self._check(rc, "gsr_band_forward")
        g = native.Gaussians()
        g.P = int(nsrc) * int(pair_cap)
        return ForwardState(cam=cam, inputs={"recv": recv}, settings=s, gauss=g, buffers=bufs, color=color,
                            radii=torch.empty(0, dtype=torch.int32, device=dev), allocs=[ag, ab, ai])

    def band_backward(self, st: ForwardState, nsrc: int, pair_cap: int, dL_dpix, reuse: dict | None = None) -> torch.Tensor:
        """B1 + per-splat 2D gradients in the received slot layout: (nsrc * pair_cap, 12) f32."""
        dpix = _f32(dL_dpix, (3, st.cam.height, st.cam.width), self.device)
        shape = (int(nsrc) * int(pair_cap), native.GSR_GRAD2D_STRIDE)
        if reuse is not None and "g2" in reuse and tuple(reuse["g2"].shape) == shape:
            out = reuse["g2"]
        else:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            if reuse is not None:
                reuse["g2"] = out
        scratch = _Allocator(self.device, reuse.setdefault("scratch", []) if reuse is not None else None)
        c = self._cam(st.cam)
        rc = self.L.gsr_band_backward(ctypes.byref(c), ctypes.byref(st.settings), int(nsrc), int(pair_cap),
                                      ctypes.byref(st.buffers), _ptr(dpix), scratch.cb, None, _ptr(out),
                                      self._stream())
        self._check(rc, "gsr_band_backward")
        return out

    def shard_backward(self, sh: ShardState, grad_recv: torch.Tensor, reuse: dict | None = None) -> dict:
        """Sum of the bands' 2D gradients per Gaussian (band order), then B2 on the shard."""
        st = ForwardState(cam=sh.cam, inputs=sh.inputs, settings=sh.settings, gauss=sh.gauss,
                          buffers=native.Buffers(), color=sh.radii, radii=sh.radii)
        if reuse is not None and reuse.get("grads_P") == sh.gauss.P:
            out, gg = reuse["grads"]
        else:
            out, gg = self._grad_tensors(st)
            if reuse is not None:
                reuse["grads_P"], reuse["grads"] = sh.gauss.P, (out, gg)
        nb = len(sh.band_rows) - 1
        rows = (ctypes.c_int32 * (nb + 1))(*[int(r) for r in sh.band_rows])
        c = self._cam(sh.cam)
        rc = self.L.gsr_shard_backward(ctypes.byref(c), ctypes.byref(sh.gauss), ctypes.byref(sh.settings), nb, rows,
                                       sh.pair_cap, _ptr(sh.state), _ptr(grad_recv.contiguous()), ctypes.byref(gg),
                                       self._stream())
        self._check(rc, "gsr_shard_backward")
        return out


# ------------------------------------------------------------------------------------------
# autograd surface (libtorch extension)
# ------------------------------------------------------------------------------------------
def ext_camera(cam: RasterCamera):
    ext = native.load_torch_ext()
    return ext.RasterCamera(cam.width, cam.height, float(cam.tanfovx), float(cam.tanfovy),
                            [float(v) for v in cam.viewmatrix], [float(v) for v in cam.projmatrix],
                            [float(v) for v in cam.campos])


def _ext_settings(ext, bg, scale_modifier, sh_degree, tile_rows, debug, max_rendered, antialiasing=False):
    y0, y1 = (0, INT32_MAX) if tile_rows is None else tile_rows
    return ext.RasterSettings([float(v) for v in bg], float(scale_modifier), int(sh_degree), int(y0), int(y1),
                              bool(debug), int(max_rendered), bool(antialiasing))


def rasterize_gaussians_aux(cam: RasterCamera, means3D, means2D, opacities, sh_dc=None, sh_rest=None,
                            colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                            sh_degree=0, scale_modifier=1.0, bg=(0.0, 0.0, 0.0), tile_rows=None, debug=False,
                            max_rendered=0, inverse_depth=False, antialiasing=False):
    """RasterizeGaussiansAux.apply: returns (color (3,H,W), depth (H,W), alpha (H,W), radii (P,)
    int32).  color, depth and alpha are differentiable in every tensor input; depth = sum w z
    (sum w / z with inverse_depth), alpha = sum w, un-normalised (expected depth = depth / alpha)."""
    ext = native.load_torch_ext()
    rs = _ext_settings(ext, bg, scale_modifier, sh_degree, tile_rows, debug, max_rendered, antialiasing)
    return ext.rasterize_gaussians_aux(ext_camera(cam), rs, bool(inverse_depth), means3D, means2D, sh_dc, sh_rest,
                                       colors_precomp, opacities, scales, rotations, cov3D_precomp)


def rasterize_gaussians(cam: RasterCamera, means3D, means2D, opacities, sh_dc=None, sh_rest=None,
                        colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                        sh_degree=0, scale_modifier=1.0, bg=(0.0, 0.0, 0.0), tile_rows=None, debug=False,
                        max_rendered=0, antialiasing=False):
    """RasterizeGaussians.apply: returns (color (3,H,W), radii (P,) int32); differentiable in
    every tensor input (means2D receives the screen-space gradient).  antialiasing: upstream's
    rasterization setting of that name (gsr.h GSR_FLAG_ANTIALIAS), carried to the backward."""
    ext = native.load_torch_ext()
    rs = _ext_settings(ext, bg, scale_modifier, sh_degree, tile_rows, debug, max_rendered, antialiasing)
    return ext.rasterize_gaussians(ext_camera(cam), rs, means3D, means2D, sh_dc, sh_rest, colors_precomp,
                                   opacities, scales, rotations, cov3D_precomp)


def depth_loss(depth, target, mask=None, alpha=None, weight=1.0, normalized=False, alpha_min=0.5,
               return_stats=False):
    """weight * mean |(pred - target) * mask| over (H, W) planes, for the "depth" / "alpha" keys of
    render(return_depth=True): pred = depth, or with `normalized` depth / alpha where
    alpha >= alpha_min (other pixels contribute nothing).  One fused HIP pass (gsr_depth_loss)
    behind a libtorch autograd Function, differentiable in depth and alpha; returns the scalar loss
    on the device (with return_stats also [weighted loss, mean |e|, contributing pixels])."""
    ext = native.load_torch_ext()
    loss, stats = ext.depth_loss(depth, alpha, target, mask, float(weight),
                                 native.DEPTH_NORMALIZED if normalized else native.DEPTH_RAW, float(alpha_min))
    return (loss, stats) if return_stats else loss


def apply_exposure(image, exposure, clamp=False):
    """Upstream's trained per-image exposure on a (3, H, W) render: out_j = sum_i exposure[i][j]
    image_i + exposure[j][3] (exposure: (3, 4), e.g. a row of the (N, 3, 4) parameter), clamped to
    [0, 1] with `clamp`.  One fused HIP pass per direction (gsr_exposure_forward / _backward) behind
    a libtorch autograd Function, differentiable in both arguments."""
    return native.load_torch_ext().apply_exposure(image, exposure, bool(clamp))


def gaussian_scores(cams, means3D, opacities, device=None, **inputs) -> dict:
    """Importance of every Gaussian over `cams`: each camera is rendered (CAbiRasterizer.forward with
    `inputs`: scales, rotations, sh_dc, ..., antialiasing, bg) and its scores accumulated in camera
    order -- "max_w" the largest blending weight T alpha the Gaussian reaches on any pixel of any
    view, "sum_w" its summed weight, "hits" the pixels it was blended into (CAbiRasterizer.scores).
    No gradients.  device: the tensors' by default."""
    cams = list(cams)
    if not cams:
        raise ValueError("gaussian_scores: no cameras")
    means3D = torch.as_tensor(means3D)
    rast = CAbiRasterizer(means3D.device if device is None else device)
    out = None
    with torch.no_grad():
        for cam in cams:
            out = rast.scores(rast.forward(cam, means3D, opacities, **inputs), into=out)
    return out


@dataclass
class PipelineParams:
    """Mirror of src/arguments/params.h:93-106."""
    convert_SHs_python: bool = False
    compute_cov3D_python: bool = False
    debug: bool = False
    antialiasing: bool = False  # upstream 3DGS's PipelineParams.antialiasing (the reference's struct has none)


def render(viewpoint_camera: RasterCamera, pc, pipe: PipelineParams, bg_color, scaling_modifier=1.0,
           override_color=None, return_depth=False, inverse_depth=False, exposure=None, clamp=False) -> dict:
    """render(): same contract as the C++ gsr::render template (csrc/torch/gsr_render.h) for a
    model exposing the reference GaussianModel getters (see model.GaussianModel).  return_depth
    adds the differentiable keys "depth" (sum w z, or sum w / z with inverse_depth) and "alpha"
    (sum w); without it the dict and the kernels launched are the colour-only ones.
    pipe.antialiasing renders with the opacity compensation (gsr.h GSR_FLAG_ANTIALIAS).
    exposure (3, 4): upstream's use_trained_exp -- "render" is apply_exposure(render, exposure, clamp);
    without one the dict and the kernels launched are unchanged."""
    from .general import eval_sh
    xyz = pc.get_xyz
    screenspace = torch.zeros_like(xyz, requires_grad=True)
    bg = [float(v) for v in torch.as_tensor(bg_color).flatten().tolist()]
    scales = rotations = cov3D = sh_dc = sh_rest = colors = None
    if pipe.compute_cov3D_python:
        cov3D = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    if override_color is not None:
        colors = override_color
    elif pipe.convert_SHs_python:
        campos = torch.as_tensor(viewpoint_camera.campos, device=xyz.device)
        dirs = xyz - campos
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        colors = torch.clamp_min(eval_sh(pc.active_sh_degree, pc.get_features, dirs) + 0.5, 0.0)
    else:
        sh_dc, sh_rest = pc.features_dc, pc.features_rest
    kw = dict(sh_dc=sh_dc, sh_rest=sh_rest, colors_precomp=colors, scales=scales, rotations=rotations,
              cov3D_precomp=cov3D, sh_degree=0 if colors is not None else pc.active_sh_degree,
              scale_modifier=scaling_modifier, bg=bg, debug=pipe.debug, antialiasing=getattr(pipe, "antialiasing", False))
    if return_depth:
        color, depth, alpha, radii = rasterize_gaussians_aux(viewpoint_camera, xyz, screenspace, pc.get_opacity,
                                                             inverse_depth=inverse_depth, **kw)
        if exposure is not None:
            color = apply_exposure(color, exposure, clamp)
        return dict(render=color, viewspace_points=screenspace, visibility_filter=radii > 0, radii=radii,
                    depth=depth, alpha=alpha)
    color, radii = rasterize_gaussians(viewpoint_camera, xyz, screenspace, pc.get_opacity, **kw)
    if exposure is not None:
        color = apply_exposure(color, exposure, clamp)
    return dict(render=color, viewspace_points=screenspace, visibility_filter=radii > 0, radii=radii)


# ------------------------------------------------------------------------------------------
# pose-differentiable render (Python autograd Function over the C ABI)
# ------------------------------------------------------------------------------------------
_posed_rasterizers: dict = {}


def _posed_rasterizer(device) -> CAbiRasterizer:
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:  # "cuda" and "cuda:0" are one device, one rasterizer
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _posed_rasterizers:
        _posed_rasterizers[dev] = CAbiRasterizer(dev)
    return _posed_rasterizers[dev]


_POSED_TENSORS = ("means3D", "means2D", "opacities", "sh_dc", "sh_rest", "colors_precomp", "scales", "rotations",
                  "cov3D_precomp")
_POSED_GRAD_KEYS = dict(means3D="means3D", means2D="means2D", opacities="opacities", sh_dc="sh_dc", sh_rest="sh_rest",
                        colors_precomp="colors", scales="scales", rotations="rotations", cov3D_precomp="cov3D")


class _RenderPosed(torch.autograd.Function):
    """forward / forward_aux of CAbiRasterizer on pose.compose(cam, delta); the backward is
    gsr_backward_posed, whose 36 camera floats are read back (one small device->host copy, which waits
    for the backward on the stream) and chained to delta in float64 on the host (pose.chain)."""

    @staticmethod
    def forward(ctx, cfg, delta, *tensors):
        from . import pose
        t = dict(zip(_POSED_TENSORS, tensors))
        rast = _posed_rasterizer(t["means3D"].device)
        cam = pose.compose(cfg["cam"], delta)
        kw = dict(scales=t["scales"], rotations=t["rotations"], sh_dc=t["sh_dc"], sh_rest=t["sh_rest"],
                  sh_degree=cfg["sh_degree"], colors_precomp=t["colors_precomp"], cov3D_precomp=t["cov3D_precomp"],
                  scale_modifier=cfg["scale_modifier"], bg=cfg["bg"], debug=cfg["debug"],
                  antialiasing=cfg["antialiasing"])
        with torch.no_grad():
            if cfg["inverse_depth"] is None:
                st = rast.forward(cam, t["means3D"], t["opacities"].reshape(-1), **kw)
            else:
                st = rast.forward_aux(cam, t["means3D"], t["opacities"].reshape(-1),
                                      inverse_depth=cfg["inverse_depth"], **kw)
        ctx.rast, ctx.st, ctx.cfg, ctx.delta = rast, st, cfg, delta.detach().clone()
        ctx.shapes = [None if x is None else tuple(x.shape) for x in tensors]
        ctx.mark_non_differentiable(st.radii)
        if cfg["inverse_depth"] is None:
            return st.color, st.radii
        return st.color, st.depth, st.alpha, st.radii

    @staticmethod
    def backward(ctx, dcolor, *rest):
        from . import pose
        st = ctx.st
        if dcolor is None:
            dcolor = torch.zeros_like(st.color)
        if ctx.cfg["inverse_depth"] is None:
            g = ctx.rast.backward(st, dcolor, camera_grad=True)
        else:
            g = ctx.rast.backward_aux(st, dcolor, rest[0], rest[1], camera_grad=True)
        ddelta = None
        if ctx.needs_input_grad[1]:
            ddelta = pose.chain(ctx.cfg["cam"], ctx.delta, g["camera"].cpu())
        grads = []
        for i, name in enumerate(_POSED_TENSORS):
            shape = ctx.shapes[i]
            grads.append(None if shape is None or not ctx.needs_input_grad[2 + i]
                         else g[_POSED_GRAD_KEYS[name]].reshape(shape))
        return (None, ddelta, *grads)


def render_posed(viewpoint_camera: RasterCamera, delta, pc, pipe: PipelineParams, bg_color, scaling_modifier=1.0,
                 override_color=None, return_depth=False, inverse_depth=False) -> dict:
    """render() of the camera pose.compose(viewpoint_camera, delta), differentiable in the Gaussians as
    render() is and in `delta`, the (6,) float64 CPU pose correction of pose.py (requires_grad for a
    gradient: d(loss)/d(delta) arrives on the CPU).  The dict is render()'s (with return_depth also
    "depth" and "alpha").  A Python autograd Function over the C ABI (CAbiRasterizer), not the libtorch
    extension: render() and the C++ gsr::render stay without pose gradients.  Each backward reads the 36
    camera floats back to the host (one small device->host copy: it synchronises the stream).  With
    pipe.convert_SHs_python or override_color the colours are inputs, so the view direction contributes
    no pose gradient (gsr.h: dL/dcampos is zero with colors_precomp)."""
    from . import pose
    from .general import eval_sh
    xyz = pc.get_xyz
    delta = torch.as_tensor(delta, dtype=torch.float64)
    if delta.device.type != "cpu" or delta.numel() != 6:
        raise ValueError("render_posed: delta is a (6,) float64 CPU tensor")
    screenspace = torch.zeros_like(xyz, requires_grad=True)
    scales = rotations = cov3D = sh_dc = sh_rest = colors = None
    if pipe.compute_cov3D_python:
        cov3D = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    if override_color is not None:
        colors = override_color
    elif pipe.convert_SHs_python:
        campos = torch.as_tensor(pose.compose(viewpoint_camera, delta).campos, device=xyz.device)
        dirs = xyz - campos
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        colors = torch.clamp_min(eval_sh(pc.active_sh_degree, pc.get_features, dirs) + 0.5, 0.0)
    else:
        sh_dc, sh_rest = pc.features_dc, pc.features_rest
    cfg = dict(cam=viewpoint_camera, sh_degree=0 if colors is not None else int(pc.active_sh_degree),
               scale_modifier=float(scaling_modifier), bg=[float(v) for v in torch.as_tensor(bg_color).flatten().tolist()],
               debug=bool(pipe.debug), antialiasing=bool(getattr(pipe, "antialiasing", False)),
               inverse_depth=bool(inverse_depth) if return_depth else None)
    out = _RenderPosed.apply(cfg, delta, xyz, screenspace, pc.get_opacity, sh_dc, sh_rest, colors, scales, rotations,
                             cov3D)
    if return_depth:
        color, depth, alpha, radii = out
        return dict(render=color, viewspace_points=screenspace, visibility_filter=radii > 0, radii=radii,
                    depth=depth, alpha=alpha)
    color, radii = out
    return dict(render=color, viewspace_points=screenspace, visibility_filter=radii > 0, radii=radii)
