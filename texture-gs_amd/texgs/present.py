"""The output stage on the device (csrc/present.hip, include/texgs_present.h): what the reference's callers do to the rasterizer's maps
before a person looks at them, each as ONE streaming HIP pass instead of a chain of torch launches, host waits and numpy / OpenCV work.

* `frame_u8`      retexture.py:28-32: clamp, composite over the background, 8-bit [H,W,3|4] (rgb or bgr) -- on the device; the copy to
                  the host is then a quarter of the float frame's bytes.  `FrameReader` overlaps that copy with the next render.
* `display`       viewer_renderer.py:138-173: the f32 [H,W,4] frame of the viewer's upload, modes rgb / norm / alpha / depth.
* `depth_colour`  train.py:22-37: masked range, normalise, colour map; no `nonzero`, no host wait, no readback.
* `to_chw01`      the clamp lines of train.py:58-71 (`affine=True`: 0.5 (n + 1) first), f32 [3,H,W].
* `cross_u8`      extract_texture.py:16-18 with `cube_map` (texture_gaussian3d.py:451-461): SH-DC texture -> 8-bit cross [3R,4R,3].

The arithmetic is a bit-exact contract, stated in numpy float32 by tests/present_ref.py: fp32, one rounding per operation, no fused
multiply-add; 8 bits by truncation of v * 255 (numpy's `astype(np.uint8)` in range), saturated outside [0, 256), NaN -> 0.

Inputs are float32, contiguous and on the GPU: everything is validated before any library call (TypeError / ValueError), then CPU
tensors raise RuntimeError -- there is no CPU fallback.  The ctypes mirrors and signatures of the header live here, as texgs/mlp.py
keeps those of texgs_mlp.h (tests/test_abi.py pins the table of texgs/_lib.py to texgs.h alone)."""
import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

PIXELS_PER_THREAD = 4               # TEXGS_PRESENT_PIXELS_PER_THREAD
PIXELS_PER_WORKGROUP = 1024         # TEXGS_PRESENT_PIXELS_PER_WORKGROUP
MAX_WORKGROUPS = 2048               # TEXGS_PRESENT_MAX_WORKGROUPS
AFFINE, COMPOSITE, SWAP_RB = 1, 2, 4        # TEXGS_PRESENT_*
MAX_CROSS_RES = 7168

_vp, _i32, _u32, _size = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t


class PresentStruct(C.Structure):
    """ctypes mirror of TexGSPresent (include/texgs_present.h)"""
    _fields_ = [("src", _vp), ("alpha", _vp), ("background", _vp), ("out_u8", _vp), ("out_hwc4", _vp), ("out_chw", _vp),
                ("height", _i32), ("width", _i32), ("channels", _i32), ("u8_channels", _i32), ("flags", _u32)]


class DepthColourStruct(C.Structure):
    """ctypes mirror of TexGSDepthColour"""
    _fields_ = [("depth", _vp), ("mask", _vp), ("lut", _vp), ("range", _vp), ("out_u8", _vp), ("out_hwc4", _vp), ("out_chw", _vp),
                ("height", _i32), ("width", _i32), ("u8_channels", _i32), ("flags", _u32)]


class CubeCrossStruct(C.Structure):
    """ctypes mirror of TexGSCubeCross"""
    _fields_ = [("texture", _vp), ("out", _vp), ("res", _i32)]


MIRRORS = {"TexGSPresent": PresentStruct, "TexGSDepthColour": DepthColourStruct, "TexGSCubeCross": CubeCrossStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_present.h
SIGNATURES = {
    "texgs_depth_colour_temp_bytes": (_size, [_i32, _i32]),
    "texgs_present": (C.c_int, [C.POINTER(PresentStruct), _vp]),
    "texgs_depth_colour": (C.c_int, [C.POINTER(DepthColourStruct), _vp, _size, _vp]),
    "texgs_cube_cross": (C.c_int, [C.POINTER(CubeCrossStruct), _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any library call ----
def _check_planar(name, t, channels=(1, 3)):
    """t: float32 contiguous [C,H,W] with C in `channels` -> (C, H, W)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dim() != 3 or t.shape[0] not in channels:
        raise ValueError(f"{name} must be [C,H,W] with C in {tuple(channels)}, got {tuple(t.shape)}")
    _check_f32(name, t)
    C_, H, W = (int(s) for s in t.shape)
    if H * W == 0 or H * W >= 2 ** 31:
        raise ValueError(f"{name}: H*W must be in [1, 2^31), got {H}x{W}")
    return C_, H, W


def _check_f32(name, t):
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_plane(name, t, H, W, allow_bool=False):
    """t: [H,W] or [1,H,W], float32 (or bool where a mask is meant), contiguous"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if tuple(t.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"{name} must be [{H},{W}] or [1,{H},{W}], got {tuple(t.shape)}")
    if allow_bool and t.dtype == torch.bool:
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return
    _check_f32(name, t)


def _check_background(background):
    if background is None or torch.is_tensor(background):
        if background is not None:
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


def _check_out(name, out, shape, dtype):
    if out is None:
        return
    if not torch.is_tensor(out):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(out).__name__}")
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")


def _check_order(order, channels):
    if order not in ("rgb", "bgr"):
        raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
    if isinstance(channels, bool) or not isinstance(channels, int):
        raise TypeError(f"channels must be an int, got {type(channels).__name__}")
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4, got {channels}")


def _check_lut(lut):
    if lut is None:
        return None
    if isinstance(lut, np.ndarray):
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError(f"lut must be uint8 [256,3], got {lut.dtype} {lut.shape}")
        return lut
    if not torch.is_tensor(lut):
        raise TypeError(f"lut must be a torch.Tensor or a numpy array, got {type(lut).__name__}")
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or not lut.is_contiguous():
        raise ValueError(f"lut must be a contiguous uint8 [256,3], got {lut.dtype} {tuple(lut.shape)}")
    return lut


def _need_gpu(what, **tensors):
    """After every other check: CPU tensors are refused (no fallback), and everything lives on one device"""
    dev = None
    for name, t in tensors.items():
        if t is None or not torch.is_tensor(t):
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"texgs.present.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the other tensors are on {dev}")
    return dev


def _background_on(background, dev):
    if background is None or torch.is_tensor(background):
        return background
    return torch.tensor(background, dtype=torch.float32, device=dev)


def _plane_f32(t):
    return None if t is None else (t.to(torch.float32) if t.dtype == torch.bool else t)       # a bool mask is converted on the device


def _lut_on(lut, dev):
    if lut is None:
        return jet_lut(dev)
    if isinstance(lut, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(lut)).to(dev)
    return lut


# ---- launches ----
def _present(src, C_, H, W, alpha, background, flags, out_u8=None, u8_channels=3, out_hwc4=None, out_chw=None):
    lib = entry()
    p = _lib.ptr
    st = PresentStruct(p(src), p(alpha), p(background), p(out_u8), p(out_hwc4), p(out_chw), H, W, C_, u8_channels, flags)
    with _lib.on(src.device) as stream:
        _lib.call(lib.texgs_present, C.byref(st), stream)


def _depth(depth, H, W, mask, lut, rng, flags=0, out_u8=None, u8_channels=3, out_hwc4=None, out_chw=None):
    lib = entry()
    p = _lib.ptr
    nbytes = lib.texgs_depth_colour_temp_bytes(H, W)
    temp = torch.empty(nbytes // 4, dtype=torch.float32, device=depth.device)
    st = DepthColourStruct(p(depth), p(mask), p(lut), p(rng), p(out_u8), p(out_hwc4), p(out_chw), H, W, u8_channels, flags)
    with _lib.on(depth.device) as stream:
        _lib.call(lib.texgs_depth_colour, C.byref(st), p(temp), nbytes, stream)


# ---- the public functions ----
def frame_u8(image, alpha=None, background=None, order="rgb", channels=3, out=None):
    """retexture.py:28-32 on the device: clamp(image, 0, 1), and with `alpha` ([H,W] or [1,H,W], float32 or bool)
    image * alpha + background * (1 - alpha), then (v * 255) truncated to uint8 -> [H,W,channels] uint8 on the device.
    `background`: 3 floats (tensor on the device, or a sequence; None is black).  `order="bgr"` swaps R and B for cv2.imwrite;
    `channels=4` appends 255.  `out` is written and returned when given.  Without alpha nothing is composited (the reference's
    all-ones mask gives the same bytes)."""
    C_, H, W = _check_planar("image", image)
    if alpha is not None:
        _check_plane("alpha", alpha, H, W, allow_bool=True)
    background = _check_background(background)
    _check_order(order, channels)
    _check_out("out", out, (H, W, channels), torch.uint8)
    dev = _need_gpu("frame_u8", image=image, alpha=alpha, background=background, out=out)
    image = image.detach()
    alpha = _plane_f32(alpha if alpha is None else alpha.detach())
    if out is None:
        out = torch.empty(H, W, channels, dtype=torch.uint8, device=dev)
    flags = (COMPOSITE if alpha is not None else 0) | (SWAP_RB if order == "bgr" else 0)
    _present(image, C_, H, W, alpha, _background_on(background, dev) if alpha is not None else None, flags, out_u8=out, u8_channels=channels)
    return out


MODES = ("rgb", "norm", "alpha", "depth")


def display(x, mode="rgb", alpha=None, lut=None, out=None):
    """viewer_renderer.py:138-173: the f32 [H,W,4] frame (4th channel 1.0) the viewer uploads.  mode "rgb": clamp(x [3,H,W]);
    "norm": clamp(0.5 (x + 1)); "alpha": x [1,H,W] or [H,W] clamped and repeated; "depth": x is the depth map [1,H,W] or [H,W],
    `alpha` its mask (None: every pixel), `lut` the colour table (default `jet_lut`).  `alpha` and `lut` are read in depth mode only."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if not torch.is_tensor(x):
        raise TypeError(f"x must be a torch.Tensor, got {type(x).__name__}")
    if mode in ("rgb", "norm"):
        C_, H, W = _check_planar("x", x, channels=(3,))
    else:
        if x.dim() == 2:
            x = x.unsqueeze(0)
        C_, H, W = _check_planar("x", x, channels=(1,))
    if mode == "depth":
        if alpha is not None:
            _check_plane("alpha", alpha, H, W, allow_bool=True)
        lut = _check_lut(lut)
    _check_out("out", out, (H, W, 4), torch.float32)
    dev = _need_gpu("display", x=x, out=out, **({"alpha": alpha, "lut": lut} if mode == "depth" else {}))
    if out is None:
        out = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
    x = x.detach()
    if mode == "depth":
        _depth(x, H, W, _plane_f32(alpha if alpha is None else alpha.detach()), _lut_on(lut, dev), None, out_hwc4=out)
    else:
        _present(x, C_, H, W, None, None, AFFINE if mode == "norm" else 0, out_hwc4=out)
    return out


def depth_colour(depth, mask=None, lut=None, as_float=True, return_range=False):
    """train.py:22-37 `normalize_depth_map`: lo / hi = min / max of the depth where mask != 0 (everywhere without a mask),
    v = clamp((d - lo) / (hi - lo + 1e-8), 0, 1), index = round-half-even(v * 255) into `lut` (uint8 [256,3] r,g,b; default `jet_lut`,
    which is NOT OpenCV's table -- see there), 0 where mask == 0.  -> f32 [3,H,W] = rgb / 255 (`as_float`), or uint8 [H,W,3];
    with `return_range` also the device tensor (lo, hi).  Nothing is read back and nothing waits for the host.  Under an all-zero mask
    the picture is black and the range is (+inf, -inf) (the reference raises); the depth under the mask must be finite."""
    if not torch.is_tensor(depth):
        raise TypeError(f"depth must be a torch.Tensor, got {type(depth).__name__}")
    if depth.dim() == 2:
        depth = depth.unsqueeze(0)
    _, H, W = _check_planar("depth", depth, channels=(1,))
    if mask is not None:
        _check_plane("mask", mask, H, W, allow_bool=True)
    lut = _check_lut(lut)
    dev = _need_gpu("depth_colour", depth=depth, mask=mask, lut=lut)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    mask = _plane_f32(mask if mask is None else mask.detach())
    if as_float:
        out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        _depth(depth.detach(), H, W, mask, _lut_on(lut, dev), rng, out_chw=out)
    else:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        _depth(depth.detach(), H, W, mask, _lut_on(lut, dev), rng, out_u8=out)
    return (out, rng) if return_range else out


def to_chw01(x, affine=False):
    """The clamp lines of train.py:58-71 for TensorBoard: clamp(x, 0, 1), or clamp(0.5 (x + 1), 0, 1) with `affine` (normal maps)
    -> a new f32 [3,H,W]; a one-channel map ([1,H,W] or [H,W]) is repeated over the three channels."""
    if torch.is_tensor(x) and x.dim() == 2:
        x = x.unsqueeze(0)
    C_, H, W = _check_planar("x", x)
    dev = _need_gpu("to_chw01", x=x)
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    _present(x.detach(), C_, H, W, None, None, AFFINE if affine else 0, out_chw=out)
    return out


def cross_u8(texture, out=None):
    """extract_texture.py:16-18 with `cube_map`: the SH-DC texture f32 [6,R,R,3] -> the 8-bit cross [3R,4R,3] (rgb), clamp(C0 x + 0.5)
    quantised; the six empty cells are zero.  One launch writes every byte: no zero fill, no float cross, nothing on the host."""
    if not torch.is_tensor(texture):
        raise TypeError(f"texture must be a torch.Tensor, got {type(texture).__name__}")
    if texture.dim() != 4 or texture.shape[0] != 6 or texture.shape[3] != 3 or texture.shape[1] != texture.shape[2]:
        raise ValueError(f"texture must be [6,R,R,3], got {tuple(texture.shape)}")
    R = int(texture.shape[1])
    if not 1 <= R <= MAX_CROSS_RES:
        raise ValueError(f"the texture resolution must be in [1,{MAX_CROSS_RES}], got {R}")
    _check_f32("texture", texture)
    _check_out("out", out, (3 * R, 4 * R, 3), torch.uint8)
    dev = _need_gpu("cross_u8", texture=texture, out=out)
    if out is None:
        out = torch.empty(3 * R, 4 * R, 3, dtype=torch.uint8, device=dev)
    lib = entry()
    st = CubeCrossStruct(texture.detach().data_ptr(), out.data_ptr(), R)
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_cube_cross, C.byref(st), stream)
    return out


# ---- the colour table ----
_jet_warned = False


def jet_table():
    """The classic piecewise-linear jet as uint8 [256,3] (r,g,b) on the host: channel = clip(1.5 - |4x - c|, 0, 1) with c = 3, 2, 1 and
    x = i / 255, times 255 and rounded half up -- in integers, clip(383 - |4i - 255c|, 0, 255), so no platform's rounding enters."""
    i = np.arange(256, dtype=np.int64)[:, None]
    c = np.array([3, 2, 1], dtype=np.int64)[None, :]
    return np.clip(383 - np.abs(4 * i - 255 * c), 0, 255).astype(np.uint8)


def jet_lut(device):
    """`jet_table()` on `device`: the default colour table of `depth_colour` and `display(mode="depth")`.

    It is NOT OpenCV's COLORMAP_JET table: cv2 is not available where this project is built and tested, so that table cannot be pinned
    here (UNPINNED; a RuntimeWarning says so once).  The colours differ by a few levels per channel.  A caller who has OpenCV gets
    its colours exactly by passing
        lut = cv2.applyColorMap(np.arange(256, dtype=np.uint8)[:, None], cv2.COLORMAP_JET)[:, 0, ::-1]
    as `lut=`."""
    global _jet_warned
    if not _jet_warned:
        _jet_warned = True
        warnings.warn("texgs.present.jet_lut is the classic piecewise-linear jet, not OpenCV's COLORMAP_JET table: that table is UNPINNED "
                      "here (cv2 cannot be imported where this project is built).  Pass lut=cv2.applyColorMap(np.arange(256, dtype=np.uint8)"
                      "[:, None], cv2.COLORMAP_JET)[:, 0, ::-1] for OpenCV's exact colours.", RuntimeWarning, stacklevel=2)
    return torch.from_numpy(jet_table()).to(device)


# ---- asynchronous readback ----
class FrameReader:
    """A ring of `capacity` pinned host buffers behind `frame_u8`, so that a view's render never waits for the previous frame's copy
    (the loop of retexture.py:25-35, which blocks on a float32 `.cpu()` per view):

        reader = FrameReader(4, H, W)
        for view in views:
            for name, frame in reader.submit(view.image_name, image, alpha=mask, background=bg):
                save(name, frame)                       # frames that had to leave the ring, oldest first
        for name, frame in reader.drain():
            save(name, frame)

    `submit` enqueues the kernel into the slot's device buffer and a non-blocking copy into its pinned buffer (through torch, so the
    caching host allocator knows the buffer is in flight), records an event and returns.  When the ring is full it first waits for the
    OLDEST slot's event and hands that frame out; a pending slot is never overwritten.  Frames come out in submission order, as
    uint8 [H,W,channels] arrays of their own (copies: the pinned buffer is reused)."""

    def __init__(self, capacity, H, W, channels=3):
        for name, v in (("capacity", capacity), ("H", H), ("W", W), ("channels", channels)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"FrameReader: {name} must be an int, got {type(v).__name__}")
        if capacity < 1:
            raise ValueError("FrameReader: capacity must be at least 1")
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"FrameReader: H*W must be in [1, 2^31), got {H}x{W}")
        if channels not in (3, 4):
            raise ValueError(f"FrameReader: channels must be 3 or 4, got {channels}")
        self.capacity, self.H, self.W, self.channels = capacity, H, W, channels
        self._dev = self._pinned = self._events = None      # allocated on the device of the first frame
        self._pending = []              # (slot, tag), oldest first
        self._next = 0

    def __len__(self):
        return len(self._pending)

    def _take_oldest(self):
        slot, tag = self._pending.pop(0)
        self._events[slot].synchronize()
        return tag, self._pinned[slot].numpy().copy()

    def submit(self, tag, image, alpha=None, background=None, order="rgb"):
        """-> the list of (tag, frame) that had to leave the ring for this one (empty until the ring is full)"""
        C_, H, W = _check_planar("image", image)
        if (H, W) != (self.H, self.W):
            raise ValueError(f"image is {H}x{W}, the reader was made for {self.H}x{self.W}")
        if alpha is not None:
            _check_plane("alpha", alpha, H, W, allow_bool=True)
        background = _check_background(background)
        _check_order(order, self.channels)
        dev = _need_gpu("FrameReader.submit", image=image, alpha=alpha, background=background)
        if self._dev is None:
            shape = (self.H, self.W, self.channels)
            self._dev = [torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(self.capacity)]
            self._pinned = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(self.capacity)]
            self._events = [torch.cuda.Event() for _ in range(self.capacity)]
        elif self._dev[0].device != dev:
            raise ValueError(f"image is on {dev}, the earlier frames were on {self._dev[0].device}")
        done = []
        if len(self._pending) == self.capacity:
            done.append(self._take_oldest())
        slot = self._next
        self._next = (slot + 1) % self.capacity
        frame_u8(image, alpha=alpha, background=background, order=order, channels=self.channels, out=self._dev[slot])
        with torch.cuda.device(dev):
            self._pinned[slot].copy_(self._dev[slot], non_blocking=True)
            self._events[slot].record(torch.cuda.current_stream(dev))
        self._pending.append((slot, tag))
        return done

    def drain(self):
        """Yield the (tag, frame) still in the ring, in submission order, waiting for each frame's own copy only"""
        while self._pending:
            yield self._take_oldest()
