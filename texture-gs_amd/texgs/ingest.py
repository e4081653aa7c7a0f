"""The input stage on the device (csrc/ingest.hip, include/texgs_ingest.h): what the reference's loaders do to a view's 8-bit files
before a loss sees them, from the uploaded BYTES -- a quarter of what the reference uploads as float32 -- in HIP passes instead of a
Pillow resize, a host division and a permute per image.

* `resize_u8`          `Image.resize(size)` for modes L and RGB: Pillow's 8-bit resample, byte for byte (bicubic, bilinear, box).
* `pil_to_torch`       utils/general.py:21-27 `PILtoTorch`: resize, / 255, [C,h,w] float32.
* `camera_images`      utils/cameras.py:103-122 and `Camera.__init__` :44-54: original_image (times the alpha mask), alpha_mask, normal.
* `composite_rgba_u8`  dataset/dataset_readers.py:219-225: RGBA over the background, 8-bit RGB.
* `resolution_for`     cameras.py:84-101: the size a view is loaded at (host integers).
* `ViewUploader`       a ring of pinned staging buffers and a side stream, so that a view's upload and decode overlap the consumer.

The arithmetic is a bit-exact contract, stated in numpy by tests/ingest_ref.py: Pillow's tap tables in IEEE double, 22-bit fixed-point
taps and int32 sums, the horizontal pass first into a clamped uint8 intermediate, an unchanged axis skipped; the decode in fp32 with
one rounding per operation; the composite in double.  The tables are built on the device: no call copies anything from the host.

Everything outside that subset raises by name, before any launch: NotImplementedError for 4 channels (Pillow premultiplies RGBA), the
other filters, `box=` and `reducing_gap=`; ValueError for shapes, dtypes, devices and limits -- there is no CPU fallback.  The ctypes
mirror and the signatures of the header live here, as texgs/present.py keeps those of texgs_present.h."""
import ctypes as C

import numpy as np
import torch

from . import _lib

BICUBIC, BILINEAR, BOX = 0, 1, 2        # TEXGS_INGEST_*
FILTERS = {"bicubic": BICUBIC, "bilinear": BILINEAR, "box": BOX}
PRECISION_BITS = 22                     # TEXGS_INGEST_PRECISION_BITS
MAX_KSIZE = 129                         # TEXGS_INGEST_MAX_KSIZE
MAX_SIDE = 16384                        # TEXGS_INGEST_MAX_SIDE
SIGNED = 1                              # TEXGS_INGEST_SIGNED

_vp, _i32, _u32, _size, _f64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t, C.c_double


class ResizeStruct(C.Structure):
    """ctypes mirror of TexGSResize (include/texgs_ingest.h)"""
    _fields_ = [("src", _vp), ("mul", _vp), ("out_u8", _vp), ("out_chw", _vp), ("out_mask", _vp), ("src_height", _i32),
                ("src_width", _i32), ("channels", _i32), ("height", _i32), ("width", _i32), ("filter", _i32), ("flags", _u32)]


MIRRORS = {"TexGSResize": ResizeStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_ingest.h
SIGNATURES = {
    "texgs_resize_ksize": (_i32, [_i32, _i32, _i32]),
    "texgs_resize_taps": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp]),
    "texgs_resize_temp_bytes": (_size, [_i32] * 6),
    "texgs_resize_u8": (C.c_int, [C.POINTER(ResizeStruct), _vp, _size, _vp]),
    "texgs_rgba_composite": (C.c_int, [_vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any launch ----
def _is_pil(x):
    return hasattr(x, "mode") and hasattr(x, "size") and hasattr(x, "resize") and not torch.is_tensor(x) and not isinstance(x, np.ndarray)


def _shape_hwc(name, shape):
    """[H,W] or [H,W,C] -> (H, W, C); C = 4 is refused by name"""
    if len(shape) not in (2, 3):
        raise ValueError(f"{name} must be [H,W] or [H,W,C], got {tuple(shape)}")
    H, W = int(shape[0]), int(shape[1])
    Cn = int(shape[2]) if len(shape) == 3 else 1
    if Cn == 4:
        raise NotImplementedError(f"{name} has 4 channels: Pillow premultiplies RGBA by its alpha before it resamples, and that is not "
                                  "built here; composite first (composite_rgba_u8) or drop the channel")
    if Cn not in (1, 3):
        raise ValueError(f"{name} must have 1 or 3 channels, got {Cn}")
    if H < 1 or W < 1:
        raise ValueError(f"{name} must not be empty, got {tuple(shape)}")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{name} is {H}x{W}: an image side above {MAX_SIDE} is not supported")
    return H, W, Cn


def _check_device_u8(name, t):
    """t: a contiguous uint8 tensor [H,W] or [H,W,C] on the GPU -> (H, W, C)"""
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a torch.Tensor on the GPU, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{name} must be torch.uint8, got {t.dtype}")
    shape = _shape_hwc(name, t.shape)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return shape


def _check_size(size):
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"size must be (width, height), got {size!r}") from None
    for v in (w, h):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"size must hold two ints, got {size!r}")
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"size must be positive, got {(w, h)}")
    if w > MAX_SIDE or h > MAX_SIDE:
        raise ValueError(f"size {(w, h)}: an image side above {MAX_SIDE} is not supported")
    return w, h


def _check_filter(filter):
    if filter is None:
        return BICUBIC                  # Image.resize without a filter
    if isinstance(filter, str) and filter.lower() in FILTERS:
        return FILTERS[filter.lower()]
    pil = {3: BICUBIC, 2: BILINEAR, 4: BOX}             # PIL.Image.Resampling values
    if not isinstance(filter, (str, bool)) and isinstance(filter, (int, np.integer)) and int(filter) in pil:
        return pil[int(filter)]
    raise NotImplementedError(f"filter {filter!r} is not built here: only {sorted(FILTERS)} (Pillow's BICUBIC, BILINEAR and BOX) are")


def _check_unsupported(box, reducing_gap):
    if box is not None:
        raise NotImplementedError("box= (resampling a region of the source) is not built here")
    if reducing_gap is not None:
        raise NotImplementedError("reducing_gap= (Pillow's two-step reduction, which changes the bytes) is not built here")


def _check_ksize(H, W, h, w, filt):
    """The library's own limits, from its host-side table (no launch): ksize of both axes"""
    lib = entry()
    for inS, outS in ((W, w), (H, h)):
        if lib.texgs_resize_ksize(inS, outS, filt) == 0:
            raise ValueError(lib.texgs_last_error().decode("utf-8", "replace"))


def _need_gpu(what, **tensors):
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.device.type != "cuda":
            raise ValueError(f"texgs.ingest.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the other tensors are on {dev}")
    return dev


def _check_out(name, out, shape, dtype):
    if out is None:
        return
    if not torch.is_tensor(out):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(out).__name__}")
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")


def _host_u8(name, image):
    """A PIL image, a uint8 array or a uint8 tensor (host or device) -> a contiguous uint8 tensor [H,W] or [H,W,C], where it is"""
    if _is_pil(image):
        if image.mode not in ("L", "RGB", "RGBA"):
            raise ValueError(f"{name} has mode {image.mode!r}; only 'L' and 'RGB' are read")
        image = np.asarray(image)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"{name} must be uint8, got {image.dtype}")
        _shape_hwc(name, image.shape)
        return torch.from_numpy(np.ascontiguousarray(image))
    if not torch.is_tensor(image):
        raise ValueError(f"{name} must be a PIL image, a numpy array or a torch.Tensor, got {type(image).__name__}")
    if image.dtype != torch.uint8:
        raise ValueError(f"{name} must be torch.uint8, got {image.dtype}")
    _shape_hwc(name, image.shape)
    return image.contiguous()


# ---- the launch ----
def _resize(src, H, W, Cn, h, w, filt, out_u8=None, out_chw=None, out_mask=None, mul=None, signed=False):
    """texgs_resize_u8 on the current stream of src's device; every tensor was checked by the caller"""
    lib = entry()
    p = _lib.ptr
    nbytes = lib.texgs_resize_temp_bytes(H, W, Cn, h, w, filt)
    if nbytes == 0:
        raise ValueError(lib.texgs_last_error().decode("utf-8", "replace"))
    with _lib.on(src.device) as stream:
        temp = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=src.device)
        st = ResizeStruct(p(src), p(mul), p(out_u8), p(out_chw), p(out_mask), H, W, Cn, h, w, filt, SIGNED if signed else 0)
        _lib.call(lib.texgs_resize_u8, C.byref(st), p(temp), nbytes, stream)


# ---- the public functions ----
def resize_u8(img, size, filter="bicubic", out=None, box=None, reducing_gap=None):
    """`PIL.Image.fromarray(img).resize(size, filter)` on the device, byte for byte: img uint8 [H,W] or [H,W,C] (C = 1 or 3) on the GPU,
    `size` = (width, height) as in Pillow -> uint8 of the same rank.  `filter`: "bicubic" (Pillow's default), "bilinear" or "box".
    `out` is written and returned when given."""
    H, W, Cn = _check_device_u8("img", img)
    w, h = _check_size(size)
    filt = _check_filter(filter)
    _check_unsupported(box, reducing_gap)
    shape = (h, w) if img.dim() == 2 else (h, w, Cn)
    _check_out("out", out, shape, torch.uint8)
    _check_ksize(H, W, h, w, filt)
    dev = _need_gpu("resize_u8", img=img, out=out)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    _resize(img, H, W, Cn, h, w, filt, out_u8=out)
    return out


def resize_taps(in_size, out_size, filter="bicubic", device="cuda"):
    """One axis of the tap tables, as the device builds them -> (taps int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, n));
    taps beyond n are 0.  (The library keeps the taps transposed, [ksize, out_size]; this returns the view with an output per row.)"""
    for name, v in (("in_size", in_size), ("out_size", out_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int, got {type(v).__name__}")
    filt = _check_filter(filter)
    lib = entry()
    ksize = lib.texgs_resize_ksize(int(in_size), int(out_size), filt)
    if ksize == 0:
        raise ValueError(lib.texgs_last_error().decode("utf-8", "replace"))
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"texgs.ingest.resize_taps: device {dev}; it runs on an AMD GPU, there is no CPU fallback")
    taps = torch.empty(ksize, int(out_size), dtype=torch.int32, device=dev)
    bounds = torch.empty(int(out_size), 2, dtype=torch.int32, device=dev)
    with _lib.on(taps.device) as stream:
        _lib.call(lib.texgs_resize_taps, int(in_size), int(out_size), filt, taps.data_ptr(), bounds.data_ptr(), stream)
    return taps.t(), bounds


def pil_to_torch(image, resolution, device="cuda"):
    """utils/general.py:21-27 `PILtoTorch`: `image.resize(resolution)` (bicubic), / 255 -> float32 [C,h,w] on `device` ([1,h,w] for a
    one-channel image).  `image`: a PIL image (mode L or RGB), or a uint8 array or tensor [H,W] / [H,W,C]; the bytes are uploaded, the
    rest happens on the device.  `resolution` = (width, height)."""
    src = _host_u8("image", image)
    H, W, Cn = _shape_hwc("image", src.shape)
    w, h = _check_size(resolution)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"texgs.ingest.pil_to_torch: device {dev}; it runs on an AMD GPU, there is no CPU fallback")
    _check_ksize(H, W, h, w, BICUBIC)
    src = src.to(dev)
    out = torch.empty(Cn, h, w, dtype=torch.float32, device=src.device)
    _resize(src, H, W, Cn, h, w, BICUBIC, out_chw=out)
    return out


def _camera_images_on(dev, image, alpha, normal, w, h, outs):
    """The kernels of camera_images from device uint8 tensors, on the current stream, into `outs` = (original, mask, normal)"""
    original, mask, nrm = outs
    if alpha is not None:       # the alpha pass first: its mask plane is the image pass's `mul`
        _resize(alpha, *_shape_hwc("alpha", alpha.shape), h, w, BICUBIC, out_mask=mask)
    _resize(image, *_shape_hwc("image", image.shape), h, w, BICUBIC, out_chw=original, mul=mask)
    if normal is not None:
        _resize(normal, *_shape_hwc("normal", normal.shape), h, w, BICUBIC, out_chw=nrm, signed=True)


def _camera_check(image, alpha, normal, resolution):
    """-> the three sources as contiguous uint8 tensors where they are, and (w, h)"""
    srcs = []
    for name, x in (("image", image), ("alpha", alpha), ("normal", normal)):
        srcs.append(None if x is None else _host_u8(name, x))
    w, h = _check_size(resolution)
    if _shape_hwc("image", srcs[0].shape)[2] != 3:
        raise ValueError(f"image must be [H,W,3], got {tuple(srcs[0].shape)}")
    if srcs[2] is not None and _shape_hwc("normal", srcs[2].shape)[2] != 3:
        raise ValueError(f"normal must be [H,W,3], got {tuple(srcs[2].shape)}")
    for name, s in zip(("image", "alpha", "normal"), srcs):
        if s is not None:
            H, W, _ = _shape_hwc(name, s.shape)
            _check_ksize(H, W, h, w, BICUBIC)
    return srcs, w, h


def _camera_outputs(srcs, w, h, dev):
    return (torch.empty(3, h, w, dtype=torch.float32, device=dev),
            None if srcs[1] is None else torch.empty(1, h, w, dtype=torch.float32, device=dev),
            None if srcs[2] is None else torch.empty(3, h, w, dtype=torch.float32, device=dev))


def camera_images(image, resolution, alpha=None, normal=None, device="cuda"):
    """utils/cameras.py:103-122 with `Camera.__init__` :44-54, from a view's 8-bit images (PIL, uint8 arrays or tensors; device
    tensors are used where they are) -> (original_image [3,h,w], alpha_mask [1,h,w] | None, normal [3,h,w] | None), float32:
        alpha_mask     = resize(alpha)[channel 0] > 0
        original_image = (resize(image) / 255) * alpha_mask          (no alpha: the reference multiplies by ones)
        normal         = (resize(normal) / 255) * 2 - 1
    each resize Pillow's bicubic to `resolution` = (width, height).  One to four launches per image (a tap table and a pass per axis
    that changes; one decode pass when none does), no host work but the upload."""
    srcs, w, h = _camera_check(image, alpha, normal, resolution)
    on_gpu = [s for s in srcs if s is not None and s.device.type == "cuda"]
    dev = on_gpu[0].device if on_gpu else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"texgs.ingest.camera_images: device {dev}; it runs on an AMD GPU, there is no CPU fallback")
    srcs = [None if s is None else s.to(dev) for s in srcs]
    _need_gpu("camera_images", image=srcs[0], alpha=srcs[1], normal=srcs[2])
    outs = _camera_outputs(srcs, w, h, srcs[0].device)
    _camera_images_on(srcs[0].device, srcs[0], srcs[1], srcs[2], w, h, outs)
    return outs


def composite_rgba_u8(rgba, background, out=None):
    """dataset/dataset_readers.py:219-225 on the device: rgba uint8 [H,W,4] over `background` (3 numbers in [0, 1]) -> uint8 [H,W,3]:
    n = b / 255.0, arr = n_c * n_a + bg_c * (1 - n_a) in float64, byte = trunc(arr * 255.0)."""
    if not torch.is_tensor(rgba):
        raise ValueError(f"rgba must be a torch.Tensor on the GPU, got {type(rgba).__name__}")
    if rgba.dtype != torch.uint8:
        raise ValueError(f"rgba must be torch.uint8, got {rgba.dtype}")
    if rgba.dim() != 3 or rgba.shape[2] != 4 or rgba.shape[0] < 1 or rgba.shape[1] < 1:
        raise ValueError(f"rgba must be [H,W,4], got {tuple(rgba.shape)}")
    if not rgba.is_contiguous():
        raise ValueError("rgba must be contiguous")
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"rgba is {H}x{W}: an image side above {MAX_SIDE} is not supported")
    try:
        bg = [float(v) for v in background]
    except (TypeError, ValueError):
        raise ValueError("background must be a sequence of 3 numbers") from None
    if len(bg) != 3 or not all(0.0 <= v <= 1.0 for v in bg):
        raise ValueError(f"background must hold 3 values in [0, 1], got {bg}")
    _check_out("out", out, (H, W, 3), torch.uint8)
    dev = _need_gpu("composite_rgba_u8", rgba=rgba, out=out)
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    lib = entry()
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_rgba_composite, rgba.data_ptr(), out.data_ptr(), H, W, bg[0], bg[1], bg[2], stream)
    return out


def resolution_for(orig_w, orig_h, resolution, resolution_scale=1.0):
    """cameras.py:84-101: the (width, height) a view of orig_w x orig_h is loaded at.  `resolution` in 1, 2, 4, 8 divides and rounds
    (Python's round: half to even); -1 keeps the size up to 1600 pixels of width and scales wider images to 1600; anything else is
    the wanted width.  Host integers only."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# ---- asynchronous upload ----
_SLOT_ALIGN = 256


class ViewUploader:
    """A ring of `capacity` pinned uint8 staging buffers, as many device uint8 buffers and ONE side stream in front of
    `camera_images`, so that the loop of cameras.py:129-135 never waits for a view's upload (the mirror of present.FrameReader):

        up = ViewUploader(4, max_h, max_w)
        for info in cam_infos:
            up.submit(info.image_name, info.image, resolution, alpha=info.alpha, normal=info.normal)
        for name, (original_image, alpha_mask, normal) in up.drain():
            ...

    `submit` copies the host arrays into a free slot's pinned buffer, enqueues the uploads and the kernels on the side stream,
    records the slot's event and returns.  A slot is taken again only after its event has completed (the host waits for that event
    alone, and only when the ring has gone round).  `drain` yields (tag, tensors) in submission order and makes the CURRENT stream
    wait for each view's event on the device; the host does not wait.  Sources are host images of at most max_h x max_w."""

    def __init__(self, capacity, max_h, max_w, device="cuda"):
        for name, v in (("capacity", capacity), ("max_h", max_h), ("max_w", max_w)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"ViewUploader: {name} must be an int, got {type(v).__name__}")
        if capacity < 1:
            raise ValueError("ViewUploader: capacity must be at least 1")
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise ValueError(f"ViewUploader: max_h and max_w must be in [1, {MAX_SIDE}], got {max_h}x{max_w}")
        self.capacity, self.max_h, self.max_w = capacity, max_h, max_w
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"ViewUploader: device {self.device}; it runs on an AMD GPU, there is no CPU fallback")
        self._image_bytes = -(-max_h * max_w * 3 // _SLOT_ALIGN) * _SLOT_ALIGN
        self._pinned = self._dev = self._events = self._stream = None       # allocated at the first submit
        self._busy = [False] * capacity
        self._pending = []              # (tag, tensors, event, slot), oldest first
        self._next = 0

    def __len__(self):
        return len(self._pending)

    def submit(self, tag, image, resolution, alpha=None, normal=None):
        srcs, w, h = _camera_check(image, alpha, normal, resolution)
        for name, s in zip(("image", "alpha", "normal"), srcs):
            if s is None:
                continue
            if s.device.type != "cpu":
                raise ValueError(f"ViewUploader.submit: {name} is on {s.device}; the uploader takes host images")
            if s.shape[0] > self.max_h or s.shape[1] > self.max_w:
                raise ValueError(f"{name} is {s.shape[0]}x{s.shape[1]}, the uploader was made for at most {self.max_h}x{self.max_w}")
        dev = self.device
        if self._pinned is None:
            n = 3 * self._image_bytes
            self._pinned = [torch.empty(n, dtype=torch.uint8).pin_memory() for _ in range(self.capacity)]
            self._dev = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(self.capacity)]
            self._events = [torch.cuda.Event() for _ in range(self.capacity)]
            self._stream = torch.cuda.Stream(device=dev)
        slot = self._next
        self._next = (slot + 1) % self.capacity
        if self._busy[slot]:
            self._events[slot].synchronize()        # the slot's own upload and kernels: its pinned bytes are free again
        with torch.cuda.device(dev):
            outs = _camera_outputs(srcs, w, h, dev)             # from the consumer stream's pool ...
            self._stream.wait_stream(torch.cuda.current_stream(dev))    # ... so whatever that memory last held is finished first
            for t in outs:
                if t is not None:
                    t.record_stream(self._stream)       # and it is not handed out again before the side stream has written it
            on_dev = []
            with torch.cuda.stream(self._stream):
                for i, s in enumerate(srcs):
                    if s is None:
                        on_dev.append(None)
                        continue
                    lo, n = i * self._image_bytes, s.numel()
                    self._pinned[slot][lo:lo + n].copy_(s.reshape(-1))
                    self._dev[slot][lo:lo + n].copy_(self._pinned[slot][lo:lo + n], non_blocking=True)
                    on_dev.append(self._dev[slot][lo:lo + n].view(s.shape))
                _camera_images_on(dev, on_dev[0], on_dev[1], on_dev[2], w, h, outs)
                self._events[slot].record(self._stream)
        self._busy[slot] = True
        self._pending.append((tag, outs, self._events[slot], slot))

    def drain(self):
        """Yield the (tag, (original_image, alpha_mask, normal)) submitted so far, in order; the current stream waits, not the host"""
        while self._pending:
            tag, outs, event, slot = self._pending.pop(0)
            torch.cuda.current_stream(self.device).wait_event(event)
            yield tag, outs
