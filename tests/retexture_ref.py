"""The statement of the retexture stage (include/texgs_retexture.h, texgs/retexture.py) in numpy; no torch, no GPU.

* `cross_new_u8`    the resized 8-bit value of every texel (or of a list of texels) of the six faces: the fp64 expressions of
                    `texture_io.resize_bilinear_u8` over the WHOLE cross, evaluated at the texels only.
* `mode_tail`       `texture_io.change_texture` per texel in float32, one rounding per operation -- the operation order that
                    reproduces tests/golden/texture_io.npz (`change_texture_m0..m4`, made from the reference's source) bit for bit.
* `latlong_f64`     latlong_to_cubemap (NVDIFFREC/util.py:103-117) and the mode arithmetic, everything in float64.
* `latlong_mixed`   the same with fp64 geometry, fp32 weights, blend and mode arithmetic: what the kernel is specified to do.

The lat-long conventions (tu = atan2(v0, -v2) / 2pi + 0.5, tv = acos(v1) / pi, bilinear at tu w - 0.5, tv h - 0.5 with BOTH axes
wrapping) are restated from the reference's source and UNPINNED against nvdiffrast."""
import numpy as np

F = np.float32
C0 = F(0.28209479177387814)
CROSS_POS = ((1, 2), (1, 0), (0, 1), (2, 1), (1, 1), (1, 3))       # texture_io._CROSS_POS
MODES = (-1, 0, 1, 2, 3)


# ---- the cross ----
def _taps(o, n_in, n_out):
    """resize_bilinear_u8's taps of one axis at the output indices o (int64)"""
    src = (o.astype(np.float64) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(src).astype(np.int64)
    f = src - i0
    i1 = np.clip(i0 + 1, 0, n_in - 1)
    f = np.where(i0 < 0, 0.0, f)
    i0 = np.clip(i0, 0, n_in - 1)
    return i0, i1, f


def all_texels(R):
    """int64 [6 R R, 3]: (f, y, x) of every texel in the texture's order"""
    f, y, x = np.meshgrid(np.arange(6), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([f.ravel(), y.ravel(), x.ravel()], -1).astype(np.int64)


def cross_new_u8(cross_u8, R, order="rgb", texels=None):
    """cross_u8 uint8 [3r,4r,3] -> the resized 8-bit `new` value, channels r, g, b: uint8 [6,R,R,3], or [n,3] for `texels`
    (int [n,3] rows of (f, y, x))"""
    cross_u8 = np.asarray(cross_u8)
    r = cross_u8.shape[0] // 3
    assert cross_u8.dtype == np.uint8 and cross_u8.shape == (3 * r, 4 * r, 3) and r >= 1
    assert order in ("rgb", "bgr")
    t = all_texels(R) if texels is None else np.asarray(texels, np.int64).reshape(-1, 3)
    pos = np.array(CROSS_POS, np.int64)
    y0, y1, fy = _taps(pos[t[:, 0], 0] * R + t[:, 1], 3 * r, 3 * R)
    x0, x1, fx = _taps(pos[t[:, 0], 1] * R + t[:, 2], 4 * r, 4 * R)
    a = cross_u8.astype(np.float64)
    fx, fy = fx[:, None], fy[:, None]
    top = a[y0, x0] * (1 - fx) + a[y0, x1] * fx
    bot = a[y1, x0] * (1 - fx) + a[y1, x1] * fx
    out = np.clip(np.floor((top * (1 - fy) + bot * fy) + 0.5), 0, 255).astype(np.uint8)
    if order == "bgr":
        out = out[:, ::-1]
    return np.ascontiguousarray(out.reshape(6, R, R, 3) if texels is None else out)


def new01_of_u8(b):
    return b.astype(F) / F(255.0)


# ---- the mode arithmetic ----
def mode_tail(old_sh0, new01, mode):
    """old_sh0, new01 float32 [..., 3] -> the new SH-DC texels, float32: every operation rounded once.  old_sh0 may be None with
    mode -1."""
    assert mode in MODES
    n = np.asarray(new01)
    assert n.dtype == F
    with np.errstate(all="ignore"):
        if mode == -1:
            v = n
        else:
            x = np.asarray(old_sh0)
            assert x.dtype == F and x.shape == n.shape
            o = np.clip(C0 * x + F(0.5), F(0), F(1))
            if mode == 0:
                c = np.clip(F(3) * o, F(0), F(1))
                v = n * (((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3))[..., None]
            elif mode == 1:
                v = n * o
            elif mode == 2:
                v = o / n
            else:
                lit = ((n[..., 0] + n[..., 1]) + n[..., 2]) > F(0.01)
                m2 = F(2) * (((o[..., 0] + o[..., 1]) + o[..., 2]) / F(3))
                v = n + np.where(lit[..., None], m2[..., None] * n, o)
        out = (v - F(0.5)) / C0
    assert out.dtype == F
    return out


def retexture_cross(old_sh0, cross_u8, mode, order="rgb"):
    """The whole cross path: old_sh0 float32 [6,R,R,3] -> float32 [6,R,R,3]"""
    return mode_tail(old_sh0, new01_of_u8(cross_new_u8(cross_u8, old_sh0.shape[1], order)), mode)


def retexture_cross_at(old_rows, cross_u8, R, mode, order, texels):
    """The cross path at a list of texels: old_rows float32 [n,3] are the old texels there"""
    return mode_tail(old_rows, new01_of_u8(cross_new_u8(cross_u8, R, order, texels)), mode)


# ---- the lat-long picture ----
def latlong_address(R, h, w):
    """fp64 geometry of every texel: (x0, x1, wx, y0, y1, wy), int64 / float64 arrays of shape [6,R,R]; both axes wrap"""
    c = (2.0 * np.arange(R, dtype=np.float64) + 1.0) / float(R) - 1.0
    gy, gx = np.meshgrid(c, c, indexing="ij")          # gy runs over rows
    one = np.ones_like(gx)
    dirs = [(one, -gy, -gx), (-one, -gy, gx), (gx, one, gy), (gx, -one, -gy), (gx, -gy, one), (-gx, -gy, -one)]     # cube_to_dir
    d = np.stack([np.stack(t, -1) for t in dirs], 0)
    v = d / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    tu = np.arctan2(v[..., 0], -v[..., 2]) / (2.0 * np.pi) + 0.5
    tv = np.arccos(np.clip(v[..., 1], -1.0, 1.0)) / np.pi

    def wrap(t, n):
        p = t * float(n) - 0.5
        fl = np.floor(p)
        i0 = np.mod(fl.astype(np.int64), n)
        return i0, np.mod(i0 + 1, n), p - fl
    x0, x1, wx = wrap(tu, w)
    y0, y1, wy = wrap(tv, h)
    return x0, x1, wx, y0, y1, wy


def _latlong(latlong, R, dt):
    pic = np.asarray(latlong)
    assert pic.ndim == 3 and pic.shape[2] == 3 and pic.dtype in (np.uint8, F)
    h, w = pic.shape[:2]
    x0, x1, wx, y0, y1, wy = latlong_address(R, h, w)
    a = pic.astype(dt) / dt(255.0) if pic.dtype == np.uint8 else pic.astype(dt)
    wx, wy = wx.astype(dt)[..., None], wy.astype(dt)[..., None]
    top = a[y0, x0] * (dt(1) - wx) + a[y0, x1] * wx
    bot = a[y1, x0] * (dt(1) - wx) + a[y1, x1] * wx
    n = top * (dt(1) - wy) + bot * wy
    assert n.dtype == dt
    return n


def latlong_mixed(latlong, R, old_sh0=None, mode=-1):
    """fp64 geometry, the weights rounded to float32 once, float32 blend and mode arithmetic -> float32 [6,R,R,3]"""
    return mode_tail(old_sh0, _latlong(latlong, R, F), mode)


def latlong_f64(latlong, R, old_sh0=None, mode=-1):
    """Everything in float64 -> float64 [6,R,R,3]"""
    n = _latlong(latlong, R, np.float64)
    c0 = 0.28209479177387814
    with np.errstate(all="ignore"):
        if mode == -1:
            v = n
        else:
            o = np.clip(c0 * np.asarray(old_sh0, np.float64) + 0.5, 0.0, 1.0)
            if mode == 0:
                v = n * np.clip(3.0 * o, 0.0, 1.0).mean(-1, keepdims=True)
            elif mode == 1:
                v = n * o
            elif mode == 2:
                v = o / n
            elif mode == 3:
                v = n + np.where((n.sum(-1) > 0.01)[..., None], 2.0 * o.mean(-1, keepdims=True) * n, o)
            else:
                raise ValueError(mode)
        return (v - 0.5) / c0


# ---- lat-long pictures that pin a convention ----
def seam_picture(h=16, w=32):
    """First column 1, last column 0, everything between 0.5: only a wrapping tap can blend the two"""
    pic = np.full((h, w, 3), F(0.5))
    pic[:, 0] = F(1.0)
    pic[:, -1] = F(0.0)
    return pic


SEAM_FACE = 4


def seam_texels(R_, h, w):
    """The texels whose tu lies within half a pixel of the seam tu = 0 | 1 -- [n, 2] rows of (y, x) on SEAM_FACE -- and their wx.
    The seam is where atan2(v0, -v2) = +-pi, that is v0 = 0 and v2 > 0: the middle column of face 4 (+z), where sphere_map's
    first and last columns look (phi = -+pi gives the direction (0, ., +sin th)); it runs on over the +z halves of faces 2 and 3.
    Faces 0, 1 and 5 (-z, where tu is around 0.5) have no such texel."""
    x0, x1, wx, *_ = latlong_address(R_, h, w)
    seam = (x0 == w - 1) & (x1 == 0)
    assert seam[SEAM_FACE].any() and not seam[[0, 1, 5]].any()
    at = np.argwhere(seam[SEAM_FACE])
    return at, wx[SEAM_FACE][at[:, 0], at[:, 1]]


FACE_COLOURS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], F) * F(0.75) + F(0.125)


def face_of(dirs):
    """The dominant-axis face of directions [..., 3]: +x, -x, +y, -y, +z, -z (cubetex's rule)"""
    a = np.abs(dirs)
    ax = np.where((a[..., 0] >= a[..., 1]) & (a[..., 0] >= a[..., 2]), 0, np.where(a[..., 1] >= a[..., 2], 1, 2))
    neg = np.take_along_axis(dirs, ax[..., None], -1)[..., 0] < 0
    return 2 * ax + neg


# ---- comparison ----
def same_class_and_bits(a, b):
    """float32 arrays: equal bit for bit where neither is a NaN, NaN exactly where the other is (a NaN's payload is no contract)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- inputs ----
def hard_cross(r, seed):
    """A random cross with NON-ZERO unused cells, black texels inside used cells (mode 2's x/0 and 0/0) and pixels whose channel sum
    is 2 and 3 (the two sides of mode 3's 0.01 threshold: 2/255 = 0.0078, 3/255 = 0.0118)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (3 * r, 4 * r, 3), dtype=np.uint8)
    n = 3 * r * 4 * r
    flat = c.reshape(n, 3)
    idx = rng.permutation(n)
    k = max(1, n // 8)
    flat[idx[:k]] = 0
    flat[idx[k:2 * k]] = (1, 1, 0)
    flat[idx[2 * k:3 * k]] = (1, 1, 1)
    flat[idx[3 * k:4 * k]] = (0, 2, 0)
    flat[idx[4 * k:5 * k]] = (3, 0, 0)
    return c


def hard_texture(R, seed):
    """SH-DC texels around the clamp's two ends, with texels that are black after sh02rgb (0/0 in mode 2)"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-2.5, 2.5, (6, R, R, 3)).astype(F)
    t[rng.random((6, R, R)) < 0.15] = F(-3.0)          # C0 x + 0.5 < 0: black
    return t
