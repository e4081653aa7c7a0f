"""The input stage's contract in numpy (include/texgs_ingest.h sections 1-3): no torch, no Pillow.

* `coeffs`, `resize`: Pillow's 8-bit resample (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the two passes) -- tap tables in
  Python floats (IEEE double, one rounding per operation), taps in 22-bit fixed point, int32 sums started at 2^21 and shifted right
  by 22, the result clamped to a byte; the horizontal pass first into a uint8 intermediate, an axis whose size does not change
  skipped.
* `decode`, `mask_plane`, `pil_to_torch`, `camera_images`: utils/general.py:21-27 and utils/cameras.py:44-54, 103-122 in float32.
* `composite`: dataset/dataset_readers.py:219-225 in float64.

Where this text and Pillow differed: nowhere.  Against Pillow 12.2.0 every case of tests/test_ingest_host.py gives the same bytes
(tests/golden/ingest.npz keeps Pillow's), and the statement of the issue needed no correction.

The inputs are made by `noise` (a 64-bit integer mix, so that they are the same on every numpy) and are not stored in the golden."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_KSIZE = 129
FILTERS = ("bicubic", "bilinear", "box")


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _box(x):
    return 1.0 if (x > -0.5 and x <= 0.5) else 0.0


_FILT = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0), "box": (_box, 0.5)}


def ksize_of(in_size, out_size, name):
    scale = in_size / out_size
    return int(math.ceil(_FILT[name][1] * max(scale, 1.0))) * 2 + 1


def coeffs(in_size, out_size, name):
    """-> (taps int32 [out_size, ksize] (0 beyond n), bounds int32 [out_size, 2] = (xmin, n))"""
    f, sup = _FILT[name]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = sup * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            p = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(p * 4194304.0 - 0.5) if p < 0 else int(p * 4194304.0 + 0.5)        # int(): C truncation
        bounds[xx] = (xmin, n)
    return kk, bounds


def _pass(img, out_size, name, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    kk, b = coeffs(src.shape[0], out_size, name)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = int(b[xx, 0]), int(b[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31                  # the sums are int32 in Pillow and on the device
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, name="bicubic"):
    """img uint8 [H,W] or [H,W,C], size = (w, h) as in Pillow -> uint8"""
    w, h = size
    H, W = img.shape[:2]
    if w != W:
        img = _pass(img, w, name, 1)
    if h != H:
        img = _pass(img, h, name, 0)
    return np.ascontiguousarray(img)


F = np.float32


def decode(b, signed=False, mul=None):
    """uint8 [h,w] or [h,w,C] -> float32 [C,h,w]: b / 255, then * 2 - 1 (signed), then * mul [h,w]"""
    if b.ndim == 2:
        b = b[:, :, None]
    v = b.astype(F) / F(255.0)
    if signed:
        v = (v * F(2.0)) - F(1.0)
    if mul is not None:
        v = v * mul.reshape(b.shape[0], b.shape[1], 1).astype(F)
    return np.ascontiguousarray(np.transpose(v, (2, 0, 1)))


def mask_plane(b):
    """uint8 [h,w] or [h,w,C] -> float32 [1,h,w]: channel 0 > 0"""
    if b.ndim == 3:
        b = b[:, :, 0]
    return (b > 0).astype(F)[None]


def pil_to_torch(img, resolution):
    return decode(resize(img, resolution))


def camera_images(image, resolution, alpha=None, normal=None):
    mask = None if alpha is None else mask_plane(resize(alpha, resolution))
    original = decode(resize(image, resolution), mul=None if mask is None else mask[0])
    nrm = None if normal is None else decode(resize(normal, resolution), signed=True)
    return original, mask, nrm


def composite(rgba, background):
    """uint8 [H,W,4], 3 numbers in [0, 1] -> uint8 [H,W,3]"""
    n = rgba.astype(np.float64) / 255.0
    bg = np.asarray(background, np.float64)
    arr = (n[:, :, :3] * n[:, :, 3:4]) + (bg * (1.0 - n[:, :, 3:4]))
    return np.trunc(arr * 255.0).astype(np.uint8)


# ---- inputs ----
def noise(shape, seed, kind="noise"):
    """uint8 of `shape`: a 64-bit integer mix of the element index and the seed; kind "binary" keeps 0 / 255 only (the bicubic
    overshoot then reaches both clamps)"""
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & (2 ** 64 - 1))     # (array arithmetic wraps)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    b = ((x >> np.uint64(24)) & np.uint64(255)).astype(np.uint8).reshape(shape)
    if kind == "binary":
        b = np.where(b & 1, np.uint8(255), np.uint8(0)).astype(np.uint8)
    return b


KINDS = ("noise", "binary")
# (source shape, (w, h)): the shapes the GPU tests use ...
GPU_CASES = [((37, 53, 3), (20, 13)), ((37, 53, 3), (53, 90)), ((31, 29), (7, 5)), ((5, 7, 3), (33, 41)), ((1, 9, 3), (4, 3)),
             ((50, 50, 3), (50, 25)), ((90, 75, 3), (1, 1)), ((300, 400, 3), (133, 100)), ((9, 1030, 3), (515, 9)),
             ((30, 25, 3), (1, 1)),
             # reductions so strong that the horizontal pass narrows its tile to keep the tile's input span in its staging buffer:
             # 50 x (bilinear, box), 128 x with one channel at the largest side (box), and the 32 x bicubic of ksize 129
             ((2, 3000, 3), (60, 2)), ((1, 16384), (128, 1)), ((2, 4160, 3), (130, 3))]
# 90 x 75 -> 1 x 1 is ksize 361 / 181 with the bicubic / bilinear filter: above the library's limit of 129, which refuses it by name
# (its box filter, ksize 91, runs); 30 x 25 -> 1 x 1 (ksize 121) is the one-pixel output every filter reaches on the device
P2T_CASES = GPU_CASES[:6] + GPU_CASES[9:10]


def fits(shape, size, name):
    """Both axes are within the library's ksize limit"""
    return max(ksize_of(shape[1], size[0], name), ksize_of(shape[0], size[1], name)) <= MAX_KSIZE
# ... and what only the statement is held to: rows of 1, 2, 3 and 5 bytes, outputs of one pixel, a non-integer ratio, more shapes
HOST_CASES = GPU_CASES + [((7, 1), (3, 4)), ((7, 2), (5, 3)), ((6, 1, 3), (4, 9)), ((7, 5), (2, 7)), ((9, 1), (1, 1)), ((1, 1, 3), (1, 1)),
                          ((12, 8, 3), (1, 5)), ((12, 8, 3), (5, 1)), ((3, 1600, 3), (533, 3)), ((64, 48, 3), (16, 16)),
                          ((120, 160, 3), (80, 60))]
TABLE_CASES = [(97, n) for n in range(1, 65)] + [(64, 97), (1600, 533), (7, 7), (4160, 130)]


def refused_tables():
    """The (in, out, filter) of TABLE_CASES whose ksize is above the library's limit: it refuses them by name instead"""
    return [(i, o, name) for i, o in TABLE_CASES for name in FILTERS if ksize_of(i, o, name) > MAX_KSIZE]


def case_key(shape, size, name, kind):
    return "resize_%s_to_%dx%d_%s_%s" % ("x".join(str(s) for s in shape), size[0], size[1], name, kind)


def case_seed(shape, size):
    return 1 + (sum((i + 1) * s for i, s in enumerate(shape)) * 31 + size[0] * 7 + size[1]) % 1000


# the views of the camera_images tests: (name, source H x W, (w, h), with alpha, with normal)
CAMERA_CASES = [("full", (37, 53), (20, 13), True, True), ("plain", (37, 53), (20, 13), False, False),
                ("alpha_only", (37, 53), (20, 13), True, False), ("skip_w", (37, 53), (53, 18), True, True),
                ("skip_h", (37, 53), (26, 37), True, True), ("same", (37, 53), (53, 37), True, True), ("up", (11, 14), (29, 23), True, True)]


def camera_inputs(H, W, seed=5):
    """-> image, alpha, normal uint8 [H,W,3]; the alpha is 0 over a corner and a stripe (a mask that zeroes pixels), small
    elsewhere too (1 and 2 are > 0)"""
    image, normal = noise((H, W, 3), seed), noise((H, W, 3), seed + 1)
    a = noise((H, W), seed + 2)
    a[:H // 3, :W // 2] = 0
    a[:, W - 3:] = 0
    a[H // 2, :] = 1
    alpha = np.repeat(a[:, :, None], 3, axis=2)
    return image, np.ascontiguousarray(alpha), normal


def composite_input():
    """uint8 [33,17,4]: every alpha extreme (0, 1, 127, 128, 254, 255) against every colour extreme, then noise"""
    rgba = noise((33, 17, 4), 77)
    ext = [0, 1, 127, 128, 254, 255]
    k = 0
    for a in ext:
        for c in ext:
            rgba[k // 17, k % 17] = (c, 255 - c, (c * 7) % 256, a)
            k += 1
    return rgba
