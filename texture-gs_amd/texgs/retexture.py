"""The retexture stage on the device (csrc/retexture.hip, include/texgs_retexture.h): the one step of the reference's retexture.py that
puts a picture INTO the texture (retexture.py:48-58 with TextureGaussian3D.change_texture, models/texture_gaussian3d.py:463-495), as
ONE streaming HIP pass over the texture instead of a float64 resize of the whole cross on the host, the upload of a float cross and
five to ten torch passes (one of them boolean-mask indexing, which waits on the host).

* `retexture_cross_u8`  an 8-bit cubemap cross [3r,4r,3] of any r -> the new SH-DC texture.  The resize is
                        `texture_io.resize_bilinear_u8` of the whole cross, evaluated only where the six faces need it, then
                        `texture_io.change_texture`: bit for bit what `change_texture(tex, load_cross_png(path, R), mode)` gives.
* `retexture_png`       the same from a PNG file: Pillow decode, upload of the BYTES, one launch.
* `retexture_latlong`   a lat-long picture [h,w,3] (the inverse of `cubetex.sphere_map`) -> the texture, after latlong_to_cubemap
                        (models/modules/NVDIFFREC/util.py:103-117): direction of every texel, tu = atan2(v0, -v2) / 2pi + 0.5,
                        tv = acos(v1) / pi, bilinear with BOTH axes wrapping, then the same mode arithmetic.  The geometry is fp64,
                        the weights are rounded to fp32 once, the blend is fp32.  These conventions are restated from the reference's
                        source and are UNPINNED against nvdiffrast (`dr.texture`'s default boundary mode), which has no ROCm build
                        to compare with; tests/retexture_ref.py holds the statement.

Modes (`texture_io.change_texture`): -1 replace; 0 modulate by the clamped 3x luminance of the old texture; 1 multiply; 2 divide old
by new (Inf and NaN as IEEE gives them); 3 tint the non-black texels of the new picture with twice the old luminance, then add.

The arithmetic is a bit-exact contract, stated in numpy by tests/retexture_ref.py: the resize in fp64, the modes in fp32, one rounding
per operation, no fused multiply-add.  `out` may be the texture itself: a texel reads only its own old texel.

The functions are NOT differentiable: inputs are detached, a texture that requires grad is accepted and the result carries no graph;
an `out` that requires grad (the model's parameter itself) is written as under torch.no_grad(), as the reference assigns `.data`.
Inputs are contiguous and on the GPU: everything is validated before any launch (TypeError / ValueError), then CPU tensors raise
RuntimeError -- there is no CPU fallback.  Everything runs on torch.cuda.current_stream(); nothing waits on the host."""
import ctypes as C

import numpy as np
import torch

from . import _lib

TEXELS_PER_THREAD = 1               # TEXGS_RETEX_TEXELS_PER_THREAD
THREADS = 256                       # TEXGS_RETEX_THREADS
MAX_RES = 7168                      # TEXGS_RETEX_MAX_RES
MAX_SRC = 16384                     # TEXGS_RETEX_MAX_SRC
ORDERS = {"rgb": 0, "bgr": 1}       # TEXGS_RETEX_RGB, TEXGS_RETEX_BGR
MODES = (-1, 0, 1, 2, 3)

_vp, _i32 = C.c_void_p, C.c_int32


class RetexCrossStruct(C.Structure):
    """ctypes mirror of TexGSRetexCross (include/texgs_retexture.h)"""
    _fields_ = [("src", _vp), ("old_tex", _vp), ("out_tex", _vp), ("r", _i32), ("R", _i32), ("mode", _i32), ("order", _i32)]


class RetexLatLongStruct(C.Structure):
    """ctypes mirror of TexGSRetexLatLong"""
    _fields_ = [("src", _vp), ("old_tex", _vp), ("out_tex", _vp), ("h", _i32), ("w", _i32), ("R", _i32), ("mode", _i32), ("src_u8", _i32)]


MIRRORS = {"TexGSRetexCross": RetexCrossStruct, "TexGSRetexLatLong": RetexLatLongStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_retexture.h
SIGNATURES = {
    "texgs_retexture_cross": (C.c_int, [C.POINTER(RetexCrossStruct), _vp]),
    "texgs_retexture_latlong": (C.c_int, [C.POINTER(RetexLatLongStruct), _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any library call ----
def _check_texture(name, t):
    """t: float32 contiguous [6,R,R,3] with 1 <= R <= MAX_RES -> R"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dim() != 4 or t.shape[0] != 6 or t.shape[3] != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"{name} must be [6,R,R,3], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    R = int(t.shape[1])
    if not 1 <= R <= MAX_RES:
        raise ValueError(f"{name}: the texture resolution must be in [1,{MAX_RES}], got {R}")
    return R


def _check_mode(mode):
    if isinstance(mode, bool) or not isinstance(mode, int):
        raise TypeError(f"mode must be an int, got {type(mode).__name__}")
    if mode not in MODES:
        raise ValueError(f"mode must be -1, 0, 1, 2 or 3, got {mode}")


def _check_cross(cross_u8):
    """cross_u8: uint8 contiguous [3r,4r,3] with 1 <= r <= MAX_SRC -> r"""
    if not torch.is_tensor(cross_u8):
        raise TypeError(f"cross_u8 must be a torch.Tensor, got {type(cross_u8).__name__}")
    if cross_u8.dtype != torch.uint8:
        raise ValueError(f"cross_u8 must be torch.uint8, got {cross_u8.dtype}")
    r = int(cross_u8.shape[0]) // 3 if cross_u8.dim() == 3 else 0
    if r < 1 or tuple(cross_u8.shape) != (3 * r, 4 * r, 3):
        raise ValueError(f"cross_u8: a cubemap cross must be [3r,4r,3], got {tuple(cross_u8.shape)}")
    if r > MAX_SRC:
        raise ValueError(f"cross_u8: r must be in [1,{MAX_SRC}], got {r}")
    if not cross_u8.is_contiguous():
        raise ValueError("cross_u8 must be contiguous")
    return r


def _check_out(out, R):
    if out is None:
        return
    if _check_texture("out", out) != R:
        raise ValueError(f"out must be [6,{R},{R},3] like the texture, got {tuple(out.shape)}")


def _need_gpu(what, **tensors):
    """After every other check: CPU tensors are refused (no fallback), and everything lives on one device"""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"texgs.retexture.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the other tensors are on {dev}")
    return dev


def _check_alias(out, old, src):
    """`out` may be the texture itself; any other shared memory is refused (the C entry point checks the same on the pointers)"""
    def overlap(a, b):
        a0, b0 = a.data_ptr(), b.data_ptr()
        return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()
    if old is not None and out.data_ptr() != old.data_ptr() and overlap(out, old):
        raise ValueError("out overlaps texture_sh0 without being the same tensor")
    if overlap(out, src):
        raise ValueError("out overlaps the picture")


# ---- the public functions ----
def retexture_cross_u8(texture_sh0, cross_u8, mode=0, order="rgb", out=None):
    """retexture.py:48-58 on the device, in one launch: the 8-bit cross `cross_u8` (uint8 [3r,4r,3], any r; `order="bgr"` when it
    holds b, g, r as cv2.imread returns it) resized to the texture's resolution as `texture_io.resize_bilinear_u8` resizes the whole
    cross, then `texture_io.change_texture(texture_sh0, cross / 255, mode)` -> the new SH-DC texture, f32 [6,R,R,3].  `out` is
    written and returned when given and may be `texture_sh0` itself (or its `.data`).  Not differentiable: inputs are detached, a
    texture that requires grad is accepted."""
    R = _check_texture("texture_sh0", texture_sh0)
    r = _check_cross(cross_u8)
    _check_mode(mode)
    if order not in ORDERS:
        raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
    _check_out(out, R)
    dev = _need_gpu("retexture_cross_u8", texture_sh0=texture_sh0, cross_u8=cross_u8, out=out)
    old, src = texture_sh0.detach(), cross_u8.detach()
    if out is None:
        out = torch.empty_like(old)
    _check_alias(out, old, src)
    st = RetexCrossStruct(src.data_ptr(), old.data_ptr(), out.data_ptr(), r, R, mode, ORDERS[order])
    lib = entry()
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_retexture_cross, C.byref(st), stream)
    return out


def retexture_latlong(latlong, R=None, texture_sh0=None, mode=-1, out=None):
    """latlong_to_cubemap (NVDIFFREC/util.py:103-117) and change_texture in one launch: the lat-long picture `latlong` (float32 in
    [0, 1] or uint8, [h,w,3], on the device; what `cubetex.sphere_map` writes) -> the new SH-DC texture, f32 [6,R,R,3].  R comes from
    `texture_sh0` or `out` when one is given, else from `R`; `texture_sh0` is needed by every mode but -1 (replace).  `out` may be
    `texture_sh0` itself.  Both axes of the picture wrap; the conventions are UNPINNED against nvdiffrast (see the module's text).
    Not differentiable: inputs are detached."""
    if not torch.is_tensor(latlong):
        raise TypeError(f"latlong must be a torch.Tensor, got {type(latlong).__name__}")
    if latlong.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"latlong must be torch.float32 or torch.uint8, got {latlong.dtype}")
    if latlong.dim() != 3 or latlong.shape[2] != 3 or not (1 <= latlong.shape[0] <= MAX_SRC and 1 <= latlong.shape[1] <= MAX_SRC):
        raise ValueError(f"latlong must be [h,w,3] with h, w in [1,{MAX_SRC}], got {tuple(latlong.shape)}")
    if not latlong.is_contiguous():
        raise ValueError("latlong must be contiguous")
    _check_mode(mode)
    sizes = {}
    if texture_sh0 is not None:
        sizes["texture_sh0"] = _check_texture("texture_sh0", texture_sh0)
    if out is not None:
        sizes["out"] = _check_texture("out", out)
    if R is not None:
        if isinstance(R, bool) or not isinstance(R, int):
            raise TypeError(f"R must be an int, got {type(R).__name__}")
        if not 1 <= R <= MAX_RES:
            raise ValueError(f"R must be in [1,{MAX_RES}], got {R}")
        sizes["R"] = R
    if not sizes:
        raise ValueError("the texture resolution is unknown: give R, texture_sh0 or out")
    if len(set(sizes.values())) > 1:
        raise ValueError("mismatched resolutions: " + ", ".join(f"{k} says {v}" for k, v in sizes.items()))
    R = next(iter(sizes.values()))
    if texture_sh0 is None and mode != -1:
        raise ValueError(f"texture_sh0 is needed by mode {mode}: only mode -1 (replace) does without the old texture")
    _check_out(out, R)
    dev = _need_gpu("retexture_latlong", latlong=latlong, texture_sh0=texture_sh0, out=out)
    old, src = (None if texture_sh0 is None else texture_sh0.detach()), latlong.detach()
    if out is None:
        out = torch.empty(6, R, R, 3, dtype=torch.float32, device=dev)
    _check_alias(out, old, src)
    h, w = int(src.shape[0]), int(src.shape[1])
    st = RetexLatLongStruct(src.data_ptr(), _lib.ptr(old), out.data_ptr(), h, w, R, mode, int(src.dtype == torch.uint8))
    lib = entry()
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_retexture_latlong, C.byref(st), stream)
    return out


def retexture_png(texture_sh0, path, mode=0, out=None):
    """`retexture_cross_u8` on a PNG file, the device form of `change_texture(texture_sh0, load_cross_png(path, R), mode)` and equal
    to it bit for bit: Pillow decode to RGB, the same 3r x 4r check (ValueError), upload of the bytes -- a twelfth of the float cross
    at the texture's resolution when r = R, less when the file is smaller --, one launch."""
    R = _check_texture("texture_sh0", texture_sh0)
    _check_mode(mode)
    _check_out(out, R)
    dev = _need_gpu("retexture_png", texture_sh0=texture_sh0, out=out)
    from PIL import Image
    img = np.array(Image.open(path).convert("RGB"))            # a copy: Pillow's buffer is read-only
    r = img.shape[0] // 3
    if img.shape != (3 * r, 4 * r, 3):
        raise ValueError(f"{path}: a cubemap cross must be 3r x 4r pixels, got {img.shape[1]} x {img.shape[0]}")
    cross = torch.from_numpy(img).to(dev)
    return retexture_cross_u8(texture_sh0, cross, mode=mode, order="rgb", out=out)
