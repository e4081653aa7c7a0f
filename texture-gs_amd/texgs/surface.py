"""The surface-point stage on the device (csrc/surface.hip, include/texgs_surface.h): the step between a rendered depth map and the UV
networks, which the reference's models run as a chain of torch launches with two or three host waits
(models/uv_map_gaussian3d.py:180-183 and :271-286, models/texture_gaussian3d.py:394-400):

    world_xyz = depth2world(depth, full_proj_transform, zfar, znear)       # arange, meshgrid, stack, linalg.inv, [HW,4] x [4,4]
    valid     = alpha.reshape(-1) > 0.5
    index     = arange(H*W)[valid];  world_xyz = world_xyz.reshape(-1, 3)[valid]

* `surface_points`  that block as three HIP launches and ONE host wait (the count): the points, their pixel indices, their alphas and
                    the pixel -> row map, in pixel order.
* `compose`         uv_map_gaussian3d.py:283-286: per-point colours back onto the pixel grid over a background, one pass, no
                    scatter_add.
* `chess_image`     `visual_step`'s chess picture: surface_points, UVNet.uv_and_jacobian, cubetex.chessboard_texture, compose.

The arithmetic is a bit-exact contract, stated in numpy by tests/surface_ref.py: the float32 projection is inverted in fp64 (adjugate
over determinant) and every point is an fp64 dot product rounded to float32 once, so the points are right to the last bit or two of
float32 where the fp32 path of `texgs.losses.depth2world` is off by 5e-5 or more.

Inputs are float32, contiguous and on the GPU: everything is validated before any library call (TypeError / ValueError), then CPU
tensors raise RuntimeError -- there is no CPU fallback.  Everything runs on torch.cuda.current_stream().  The ctypes mirrors and
signatures of the header live here, as texgs/present.py keeps those of texgs_present.h."""
import ctypes as C
import math

import torch

from . import _lib

PIXELS_PER_THREAD = 4               # TEXGS_SURFACE_PIXELS_PER_THREAD
PIXELS_PER_WORKGROUP = 1024         # TEXGS_SURFACE_PIXELS_PER_WORKGROUP
SCAN_WIDTH = 256                    # TEXGS_SURFACE_SCAN_WIDTH
MAX_SIDE = 16384                    # TEXGS_SURFACE_MAX_SIDE

_vp, _i32, _u32, _f32, _f64, _size = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_double, C.c_size_t


class SurfacePointsStruct(C.Structure):
    """ctypes mirror of TexGSSurfacePoints (include/texgs_surface.h)"""
    _fields_ = [("depth", _vp), ("alpha", _vp), ("full_proj", _vp), ("xyz", _vp), ("index", _vp), ("alpha_sel", _vp), ("rank", _vp),
                ("count", _vp), ("zfar", _f64), ("znear", _f64), ("threshold", _f32), ("height", _i32), ("width", _i32), ("capacity", _i32)]


class SurfaceComposeStruct(C.Structure):
    """ctypes mirror of TexGSSurfaceCompose"""
    _fields_ = [("values", _vp), ("rank", _vp), ("alpha", _vp), ("background", _vp), ("out", _vp), ("rows", _i32), ("height", _i32),
                ("width", _i32)]


MIRRORS = {"TexGSSurfacePoints": SurfacePointsStruct, "TexGSSurfaceCompose": SurfaceComposeStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_surface.h
SIGNATURES = {
    "texgs_surface_temp_bytes": (_size, [_i32, _i32]),
    "texgs_surface_points": (C.c_int, [C.POINTER(SurfacePointsStruct), _vp, _size, _vp]),
    "texgs_surface_compose": (C.c_int, [C.POINTER(SurfaceComposeStruct), _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any library call ----
def _check_f32(name, t):
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_map(name, t, shape=None):
    """t: float32 contiguous [H,W] or [1,H,W] (of `shape` when given) -> (H, W)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)):
        raise ValueError(f"{name} must be [H,W] or [1,H,W], got {tuple(t.shape)}")
    H, W = int(t.shape[-2]), int(t.shape[-1])
    if shape is not None and (H, W) != shape:
        raise ValueError(f"{name} must be [{shape[0]},{shape[1]}] or [1,{shape[0]},{shape[1]}], got {tuple(t.shape)}")
    _check_f32(name, t)
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{name}: each side must be in [1,{MAX_SIDE}], got {H}x{W}")
    return H, W


def _check_number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    return float(v)


def _check_camera(full_proj_transform, zfar, znear):
    if not torch.is_tensor(full_proj_transform):
        raise TypeError(f"full_proj_transform must be a torch.Tensor, got {type(full_proj_transform).__name__}")
    if tuple(full_proj_transform.shape) != (4, 4):
        raise ValueError(f"full_proj_transform must be [4,4], got {tuple(full_proj_transform.shape)}")
    _check_f32("full_proj_transform", full_proj_transform)
    zfar, znear = _check_number("zfar", zfar), _check_number("znear", znear)
    if math.isnan(zfar) or math.isnan(znear) or zfar == znear:
        raise ValueError(f"zfar and znear must be two different numbers, got {zfar} and {znear}")
    return zfar, znear


def _check_background(background):
    if background is None:
        return None
    if torch.is_tensor(background):
        if background.numel() != 3:
            raise ValueError(f"background must hold 3 values, got shape {tuple(background.shape)}")
        _check_f32("background", background)
        return background
    try:
        vals = [float(v) for v in background]
    except (TypeError, ValueError):
        raise TypeError("background must be a tensor or a sequence of 3 numbers") from None
    if len(vals) != 3:
        raise ValueError(f"background must hold 3 values, got {len(vals)}")
    return vals


def _need_gpu(what, **tensors):
    """After every other check: CPU tensors are refused (no fallback), and everything lives on one device"""
    dev = None
    for name, t in tensors.items():
        if t is None or not torch.is_tensor(t):
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"texgs.surface.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the other tensors are on {dev}")
    return dev


# ---- the result ----
class SurfacePoints:
    """What `surface_points` returns.  `count` = M, the number of selected pixels; `xyz` f32 [M,3], `index` int64 [M] (the pixels,
    ascending), `alpha` f32 [M] and `rank` int32 [H,W] (pixel -> row, -1 where not selected); the ones not asked for are None.
    xyz, index and alpha are the [:M] prefixes of buffers of H*W rows.  Made with wait=False, the object waits for the count on the
    first access of `count`, `xyz`, `index` or `alpha`; `rank`, `height` and `width` never wait."""

    def __init__(self, height, width, xyz, index, alpha, rank, pinned, event):
        self.height, self.width, self.rank = height, width, rank
        self._xyz, self._index, self._alpha = xyz, index, alpha
        self._pinned, self._event, self._count = pinned, event, None

    def wait(self):
        """Block until the count has landed (once); returns it"""
        if self._count is None:
            self._event.synchronize()
            self._count = int(self._pinned[0]) & 0xFFFFFFFF
            _PIN_POOL.append(self._pinned)
            self._pinned = self._event = None
        return self._count

    @property
    def count(self):
        return self.wait()

    @property
    def xyz(self):
        return self._xyz[:self.wait()]

    @property
    def index(self):
        return None if self._index is None else self._index[:self.wait()]

    @property
    def alpha(self):
        return None if self._alpha is None else self._alpha[:self.wait()]


def surface_points(depth, alpha, full_proj_transform, zfar, znear, threshold=0.5, with_index=True, with_alpha=False, with_rank=False,
                   wait=True):
    """The world points of the pixels with alpha > threshold, in pixel order -> SurfacePoints.

    depth, alpha: f32 [H,W] or [1,H,W] (detached); full_proj_transform: f32 [4,4] on the device, the reference's row-vector
    convention (clip = [p, 1] @ P); zfar, znear: numbers, zfar != znear; threshold: a number, compared as float32 (strict, so a NaN
    alpha is not selected).  `with_index` / `with_alpha` / `with_rank` add the pixel indices, the selected alphas and the
    pixel -> row map.  The one host wait is for the count: a pinned word, an event.  With wait=False it is left to the first access of
    the result, so the caller can queue other work first.  No selected pixel gives empty tensors, not an error.  A singular
    projection gives non-finite points and is not checked."""
    H, W = _check_map("depth", depth)
    _check_map("alpha", alpha, (H, W))
    zfar, znear = _check_camera(full_proj_transform, zfar, znear)
    threshold = _check_number("threshold", threshold)
    if math.isnan(threshold):
        raise ValueError("threshold is NaN")
    dev = _need_gpu("surface_points", depth=depth, alpha=alpha, full_proj_transform=full_proj_transform)
    lib = entry()
    depth, alpha, proj = depth.detach(), alpha.detach(), full_proj_transform.detach()
    n = H * W
    p = _lib.ptr
    with _lib.on(dev) as stream:
        xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
        index = torch.empty(n, dtype=torch.int64, device=dev) if with_index else None
        alpha_sel = torch.empty(n, dtype=torch.float32, device=dev) if with_alpha else None
        rank = torch.empty(H, W, dtype=torch.int32, device=dev) if with_rank else None
        count = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = lib.texgs_surface_temp_bytes(H, W)
        temp = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        st = SurfacePointsStruct(p(depth), p(alpha), p(proj), p(xyz), p(index), p(alpha_sel), p(rank), p(count), zfar, znear, threshold,
                                 H, W, n)
        _lib.call(lib.texgs_surface_points, C.byref(st), p(temp), nbytes, stream)
        pinned = _pin_take()
        pinned.copy_(count, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(dev))
    out = SurfacePoints(H, W, xyz, index, alpha_sel, rank, pinned, event)
    if wait:
        out.wait()
    return out


_PIN_POOL = []          # pinned words whose copy has landed (SurfacePoints.wait gives them back)


def _pin_take():
    """One pinned word per call in flight"""
    return _PIN_POOL.pop() if _PIN_POOL else torch.empty(1, dtype=torch.int32).pin_memory()


def compose(points, values, alpha, background=None):
    """uv_map_gaussian3d.py:283-286 in one pass: out[c,p] = background[c] * (1 - alpha[p]) + alpha[p] * values[rank[p]][c] on the
    selected pixels and the first term alone elsewhere -> f32 [3,H,W].  points: a SurfacePoints made with_rank=True; values: f32
    [M,3], a colour per point; alpha: the map the points were selected from; background: 3 floats (device tensor, or a sequence; None
    is black)."""
    if not isinstance(points, SurfacePoints):
        raise TypeError(f"points must be a SurfacePoints, got {type(points).__name__}")
    if points.rank is None:
        raise ValueError("points carries no rank map: make it with surface_points(..., with_rank=True)")
    H, W = points.height, points.width
    _check_map("alpha", alpha, (H, W))
    if not torch.is_tensor(values):
        raise TypeError(f"values must be a torch.Tensor, got {type(values).__name__}")
    if values.dim() != 2 or values.shape[1] != 3:
        raise ValueError(f"values must be [M,3], got {tuple(values.shape)}")
    _check_f32("values", values)
    background = _check_background(background)
    dev = _need_gpu("compose", rank=points.rank, values=values, alpha=alpha, background=background)
    M = points.count
    if int(values.shape[0]) != M:
        raise ValueError(f"values has {int(values.shape[0])} rows, the points are {M}")
    if background is not None and not torch.is_tensor(background):
        background = torch.tensor(background, dtype=torch.float32, device=dev)
    lib = entry()
    p = _lib.ptr
    values, alpha = values.detach(), alpha.detach()
    with _lib.on(dev) as stream:
        out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        st = SurfaceComposeStruct(p(values) if M else None, p(points.rank), p(alpha), p(background), p(out), M, H, W)
        _lib.call(lib.texgs_surface_compose, C.byref(st), stream)
    return out


def chess_image(depth, alpha, full_proj_transform, zfar, znear, uv_net, geo_emb, background=None):
    """`visual_step`'s chess picture (uv_map_gaussian3d.py:271-286) -> f32 [3,H,W]: the surface points of the render, their UVs from
    `uv_net` (texgs.uvnet.UVNet, fused kernel), the chessboard's colours there, composited over `background` (None: black, as the
    reference has it).  geo_emb: the [128] embedding vector."""
    from . import cubetex
    from .uvmap import _emb_vector
    pts = surface_points(depth, alpha, full_proj_transform, zfar, znear, with_index=False, with_rank=True)
    if pts.count == 0:
        return compose(pts, pts.xyz, alpha, background)
    with torch.no_grad():
        uv, _ = uv_net.uv_and_jacobian(pts.xyz, _emb_vector(geo_emb))
        rgb = cubetex.chessboard_texture(uv).reshape(-1, 3).contiguous()
    return compose(pts, rgb, alpha, background)
