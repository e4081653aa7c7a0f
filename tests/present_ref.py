"""The statement of the output stage (include/texgs_present.h, texgs/present.py) in numpy float32, operation by operation -- every
product, sum and quotient below is ONE float32 operation, in the order the header lists them -- and, next to it, the reference's own
lines restated in torch-CPU float32 (retexture.py:28-32, train.py:28-37, viewer_renderer.py:138-173, cube_map with
extract_texture.py:17).  tests/test_present_host.py holds the two equal on the inputs built here, which pins the statement to the
reference; tests/test_present_gpu.py holds the kernels equal to the statement, bit for bit.

Where the reference leaves a value open the statement defines it: 8 bits saturate outside [0, 256) and NaN gives 0 (numpy's
`astype(np.uint8)` is undefined there); the clamp is by comparison, so -0 stays -0 (torch.clamp may give either zero: the two are
compared as VALUES there); an all-zero mask gives a black picture and the range (+inf, -inf) (the reference raises)."""
import numpy as np
import torch

F = np.float32
SH_C0 = F(0.28209479177387814)
CROSS_CELLS = {(0, 1): 2, (1, 0): 1, (1, 1): 4, (1, 2): 0, (1, 3): 5, (2, 1): 3}       # (row, column) -> face, cube_map :455-460


# ---- the statement ----
def clamp01(v):
    """torch.clamp(v, 0, 1) by comparison: a NaN stays NaN, -0 stays -0"""
    v = np.asarray(v, dtype=F)
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def quantise(v):
    """(uint8) trunc(v * 255.0f); below 0 and NaN -> 0, 256 and above -> 255"""
    t = np.asarray(v, dtype=F) * F(255)
    with np.errstate(invalid="ignore"):
        safe = np.where((t > 0) & (t < 256), t, F(0))
        return np.where(t > 0, np.where(t < 256, np.trunc(safe), 255), 0).astype(np.uint8)


def present_values(src, alpha=None, background=None, affine=False, composite=False):
    """src f32 [C,H,W], C in {1, 3} -> v f32 [3,H,W]"""
    src = np.asarray(src, dtype=F)
    v = np.broadcast_to(src, (3,) + src.shape[1:]).copy()
    if affine:
        v = F(0.5) * (v + F(1))
    v = clamp01(v)
    if composite:
        a = np.asarray(alpha, dtype=F).reshape(1, *src.shape[1:])
        bg = np.zeros(3, F) if background is None else np.asarray(background, dtype=F)
        v = (v * a) + (bg.reshape(3, 1, 1) * (F(1) - a))
    return v.astype(F)


def u8_frame(rgb_u8, channels=3, order="rgb"):
    """bytes [3,H,W] -> [H,W,channels], bgr on request, the 4th channel 255"""
    hwc = np.ascontiguousarray(np.transpose(rgb_u8, (1, 2, 0)))
    if order == "bgr":
        hwc = hwc[:, :, ::-1]
    if channels == 4:
        hwc = np.concatenate([hwc, np.full(hwc.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(hwc)


def hwc4(v):
    """f32 [3,H,W] -> f32 [H,W,4], the 4th channel 1.0"""
    hwc = np.transpose(v, (1, 2, 0))
    return np.ascontiguousarray(np.concatenate([hwc, np.ones(hwc.shape[:2] + (1,), F)], axis=2))


def frame_u8(image, alpha=None, background=None, order="rgb", channels=3):
    v = present_values(image, alpha, background, composite=alpha is not None)
    return u8_frame(quantise(v), channels, order)


def depth_colour(depth, mask, lut):
    """depth f32 [H,W], mask f32 [H,W] or None, lut u8 [256,3] -> (rgb bytes [3,H,W], (lo, hi) as float32)"""
    d = np.asarray(depth, dtype=F)
    on = np.ones(d.shape, bool) if mask is None else (np.asarray(mask) != 0)
    lo = d[on].min() if on.any() else F(np.inf)
    hi = d[on].max() if on.any() else F(-np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = clamp01((d - lo) / ((hi - lo) + F(1e-8)))
        t = np.abs(v * F(255))
        idx = np.where(t >= 255, 255, np.where(t > 0, np.rint(np.where(t > 0, t, F(0))), 0)).astype(np.int64)       # NaN -> 0
    rgb = np.asarray(lut)[idx]                                       # [H,W,3]
    rgb = np.where(on[:, :, None], rgb, 0).astype(np.uint8)
    return np.ascontiguousarray(np.transpose(rgb, (2, 0, 1))), (F(lo), F(hi))


def bytes_as_float(rgb_u8):
    return (rgb_u8.astype(F) / F(255)).astype(F)


def cross_u8(texture):
    """f32 [6,R,R,3] -> u8 [3R,4R,3]"""
    tex = np.asarray(texture, dtype=F)
    R = tex.shape[1]
    q = quantise(clamp01((tex * SH_C0) + F(0.5)))
    out = np.zeros((3 * R, 4 * R, 3), np.uint8)
    for (cy, cx), face in CROSS_CELLS.items():
        out[cy * R:(cy + 1) * R, cx * R:(cx + 1) * R] = q[face]
    return out


# ---- the reference's own lines, torch-CPU float32 ----
def reference_retexture(image, gt_alpha, background):
    """retexture.py:28-32; image [3,H,W], gt_alpha [1,H,W] or None, background [3], all torch float32"""
    image = torch.clamp(image, 0.0, 1.0)
    H, W = image.shape[1], image.shape[2]
    gt_alpha = gt_alpha if gt_alpha is not None else torch.ones((1, H, W)).float()
    image = image * gt_alpha.repeat(3, 1, 1) + background[:, None, None].expand_as(image) * (1 - gt_alpha.repeat(3, 1, 1))
    return (image.permute(1, 2, 0).detach().cpu().numpy() * 255).astype(np.uint8).copy()


def reference_depth(depth, mask, lut):
    """train.py:22-37 (viewer_renderer.py:150-165 is the same with a mask); depth [1,H,W], mask [1,H,W] or None.  OpenCV's two
    calls are restated: convertScaleAbs is saturate_cast<uchar>(|x|) with cvRound (round half to even), applyColorMap + cvtColor is a
    table look-up, here np.take on `lut` (r,g,b)."""
    depth = depth.squeeze(0)
    if mask is not None:
        mask = mask.bool().squeeze(0)
    min_d = torch.min(depth[mask]) if mask is not None else torch.min(depth)
    max_d = torch.max(depth[mask]) if mask is not None else torch.max(depth)
    depth = (depth - min_d) / (max_d - min_d + 1e-8)
    depth = torch.clamp(depth, 0.0, 1.0)
    scaled = np.clip(np.rint(np.abs(depth.detach().cpu().numpy() * 255)), 0, 255).astype(np.uint8)
    d_color = np.take(np.asarray(lut), scaled, axis=0)
    d_color = torch.tensor(d_color)
    if mask is not None:
        d_color[~mask] = 0
    return (d_color.float() / 255).permute(2, 0, 1)


def reference_viewer(visual_pkg, render_mode, lut=None):
    """viewer_renderer.py:138-173 -> the contiguous [H,W,4] frame"""
    if render_mode == 'rgb':
        img = torch.clamp(visual_pkg['image'], 0.0, 1.0)
    elif render_mode == 'norm':
        img = torch.clamp(0.5 * (visual_pkg['norm'] + 1.), 0.0, 1.0)
    elif render_mode == 'alpha':
        img = torch.clamp(visual_pkg['alpha'].repeat(3, 1, 1), 0.0, 1.0)
    elif render_mode == 'depth':
        img = torch.clamp(reference_depth(visual_pkg['depth'], visual_pkg['alpha'], lut), 0.0, 1.0)
    else:
        raise NotImplementedError
    img = img.permute(1, 2, 0)
    img = torch.concat([img, torch.ones_like(img[..., :1])], dim=-1)
    return img.contiguous()


def reference_cross(texture):
    """sh02rgb, cube_map (texture_gaussian3d.py:19-21, 451-461) and extract_texture.py:17; texture torch f32 [6,R,R,3]"""
    rgb = torch.clamp(0.28209479177387814 * texture + 0.5, 0.0, 1.0)
    res = texture.shape[1]
    cubemap = torch.zeros((res * 3, res * 4, 3), dtype=rgb.dtype)
    cubemap[0:res, res:2 * res, :] = rgb[2]
    cubemap[res:2 * res, 0:res, :] = rgb[1]
    cubemap[res:2 * res, res:2 * res, :] = rgb[4]
    cubemap[res:2 * res, 2 * res:3 * res, :] = rgb[0]
    cubemap[res:2 * res, 3 * res:4 * res, :] = rgb[5]
    cubemap[2 * res:3 * res, res:2 * res, :] = rgb[3]
    return (torch.clamp(cubemap, 0, 1) * 255).detach().cpu().numpy().astype(np.uint8)


# ---- inputs (shared by the host and the GPU tests) ----
def planted_values():
    """Where truncation, the clamp and the saturation can go wrong: the zeros, 1, the float32 neighbours of k/255, 1 - 2^-24, 256/255"""
    vals = [F(0), F(-0.0), F(1), F(1) - F(2.0 ** -24), F(256) / F(255)]
    for k in (1, 2, 3, 85, 127, 128, 170, 254, 255):
        x = F(k) / F(255)
        vals += [np.nextafter(x, F(-1)), x, np.nextafter(x, F(2))]
    return np.array(vals, dtype=F)


def make_image(C, H, W, seed, affine=False):
    """Seeded noise in [-0.2, 1.2] with the planted values at the front of every plane (as many as fit).  For the affine mode the
    planted values are mapped to 2 v - 1 (exact up to one rounding; the statement and the kernel see the same input either way)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.2, 1.2, (C, H * W)).astype(F)
    pv = planted_values()
    if affine:
        img = (F(2) * img - F(1)).astype(F)
        pv = (F(2) * pv - F(1)).astype(F)
    n = min(pv.size, H * W)
    for c in range(C):
        img[c, :n] = np.roll(pv, c)[:n]
    return img.reshape(C, H, W)


def make_alpha(H, W):
    """0, 1, 0.5, 1/3 in turn"""
    a = np.array([0, 1, 0.5, 1.0 / 3.0], dtype=F)
    return np.resize(a, H * W).reshape(H, W).copy()


BACKGROUND = np.array([0.1, 0.7, 0.33], dtype=F)


def make_depth(H, W, seed):
    return np.random.default_rng(seed).uniform(0.5, 7.0, (H, W)).astype(F)


def near_tie_depth():
    """lo = 0, hi = 255 and d = k + 0.5: v * 255 lands next to the ties of rint"""
    d = np.concatenate([[0.0, 255.0], np.arange(255) + 0.5, np.arange(256)]).astype(F)
    return d.reshape(1, -1)


def random_lut(seed=11):
    return np.random.default_rng(seed).integers(0, 256, (256, 3), dtype=np.uint8)


def make_texture(R, seed):
    """SH-DC values whose colours cover [below 0, above 1], with exact byte boundaries planted"""
    rng = np.random.default_rng(seed)
    tex = rng.uniform(-2.2, 2.2, (6, R, R, 3)).astype(F)
    pv = ((planted_values() - F(0.5)) / SH_C0).astype(F)
    flat = tex.reshape(-1)
    n = min(pv.size, flat.size)
    flat[:n] = pv[:n]
    return tex
