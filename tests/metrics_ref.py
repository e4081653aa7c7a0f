"""The statement of the evaluation metrics (texgs.metrics, csrc/metrics.hip) in float64 numpy / scipy.

skimage is not installed where this project is developed, so `ssim_map` RESTATES the algorithm of
skimage.metrics.structural_similarity (channel_axis=0, data_range=1.0, default window) from its published definition; it is not
pinned to skimage's output:
    ux, uy, uxx, uyy, uxy = scipy.ndimage.uniform_filter(., size=7) of x, y, x x, y y, x y
    vx = cov_norm (uxx - ux ux), vy likewise, vxy = cov_norm (uxy - ux uy),  cov_norm = 49 / 48  (sample covariance)
    S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = 0.01^2, C2 = 0.03^2
    mean of S cropped by 3 on every side (the filter's border mode never reaches the mean), then the mean over channels.
The reference hands skimage float32 arrays, so ITS window arithmetic is float32; this statement, like the kernel, is float64.

`d` is the fp32 subtraction cast to float64, as utils/metrics.py:19,22 and losses/pixelwise_loss.py subtract in fp32.
`mae` is utils/metrics.py:25-37 with cos = x.y / (max(|x|, 1e-6) max(|y|, 1e-6)) (torch.cosine_similarity, eps = 1e-6) clamped to
[-1, 1]: the reference's bounds +-(1 - 1e-10) round to +-1 in float32."""
import os

import numpy as np

C1, C2, COV_NORM, WIN, PAD = 0.01 ** 2, 0.03 ** 2, 49.0 / 48.0, 7, 3
ROW = 16


def clamp01(a):
    return np.clip(a, np.float32(0.0), np.float32(1.0))


def ssim_map(x, y):
    """x, y [H, W] -> S [H, W] float64 (uncropped)"""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    f = lambda a: uniform_filter(a, size=WIN)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim_channel_sums(x, y):
    """[3, H, W] pair -> sum of S over the cropped map, per channel"""
    if x.shape[-1] < WIN or x.shape[-2] < WIN:
        raise ValueError("win_size exceeds image extent")
    return np.array([ssim_map(x[c], y[c])[PAD:-PAD, PAD:-PAD].sum() for c in range(x.shape[0])])


def ssim(x, y):
    H, W = x.shape[-2:]
    return float(np.mean(ssim_channel_sums(x, y) / ((H - 2 * PAD) * (W - 2 * PAD))))


def diff(x, y):
    return (np.asarray(x, np.float32) - np.asarray(y, np.float32)).astype(np.float64)


def mse(x, y):
    d = diff(x, y)
    return (d * d).reshape(d.shape[0], -1).mean(axis=1, keepdims=True)


def psnr(x, y):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(mse(x, y)))


def l1(x, y):
    return float(np.abs(diff(x, y)).mean())


def angles_deg(n1, n2, eps=1e-6):
    """[3, H, W] pair -> [H, W] degrees"""
    a, b = np.asarray(n1, np.float64), np.asarray(n2, np.float64)
    sa, sb = (a * a).sum(0), (b * b).sum(0)
    na, nb = np.sqrt(sa), np.sqrt(sb)
    # the same number as max(na, eps) max(nb, eps); where no norm is clamped |a| |b| is taken as sqrt(sa sb), which is sa exactly
    # for a = b: identical normals then give cos = 1 and 0 degrees, not the 1e-6 degrees of an ulp below 1
    den = np.where((na >= eps) & (nb >= eps), np.sqrt(sa * sb), np.maximum(na, eps) * np.maximum(nb, eps))
    cos = np.clip((a * b).sum(0) / den, -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def mae(n1, n2, alpha=None):
    deg = angles_deg(n1, n2)
    if alpha is None:
        return float(deg.mean())
    a = np.asarray(alpha, np.float64).reshape(deg.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64((deg * a).sum()) / np.float64(a.sum()))


def row(image, gt, norm=None, gt_norm=None, alpha=None, clamp=False):
    """The 16 values csrc/metrics.hip leaves for one view (include/texgs.h TEXGS_METRICS_*)"""
    image, gt = np.asarray(image, np.float32), np.asarray(gt, np.float32)
    if clamp:
        image, gt = clamp01(image), clamp01(gt)
    H, W = image.shape[-2:]
    d = diff(image, gt)
    r = np.zeros(ROW, np.float64)
    r[0] = np.abs(d).sum()
    r[1:4] = (d * d).reshape(3, -1).sum(axis=1)
    r[4:7] = ssim_channel_sums(image, gt)
    if norm is not None:
        deg = angles_deg(norm, gt_norm)
        a = np.ones_like(deg) if alpha is None else np.asarray(alpha, np.float64).reshape(deg.shape)
        r[7], r[8] = (deg * a).sum(), a.sum()
    r[9], r[10] = H * W, (H - 2 * PAD) * (W - 2 * PAD)
    return r


# ---- seeded inputs shared by the host and the GPU tests ----
SHAPES = [(7, 7), (8, 9), (33, 65), (38, 70), (64, 64), (100, 75)]
KINDS = ["noise", "smooth", "flat", "identical", "out_of_range"]


def image_pair(kind, H, W, seed=0):
    """-> (image, gt) float32 [3, H, W]"""
    rng = np.random.RandomState(1000 * seed + 7 * H + W)
    if kind == "noise":
        x, y = rng.rand(3, H, W), rng.rand(3, H, W)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([0.5 + 0.4 * np.sin(0.31 * xx + 0.17 * yy + c) * np.cos(0.11 * yy - 0.05 * xx * c) for c in range(3)])
        x, y = base + 0.02 * rng.randn(3, H, W), base + 0.02 * rng.randn(3, H, W)
    elif kind == "flat":                    # the cancellation case: uxx - ux ux is ~1e-5 of its terms
        x, y = 0.8 + 0.005 * (2 * rng.rand(3, H, W) - 1), 0.8 + 0.005 * (2 * rng.rand(3, H, W) - 1)
    elif kind == "identical":
        x = rng.rand(3, H, W)
        y = x.copy()
    elif kind == "out_of_range":            # about a third of the values outside [0, 1] on either side
        x, y = 1.5 * rng.rand(3, H, W) - 0.25, 1.5 * rng.rand(3, H, W) - 0.25
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def normal_pair(H, W, seed=0, min_deg=5.0, max_deg=60.0):
    """Unit normals and a second map rotated away from them by min_deg .. max_deg about a random perpendicular axis, and an alpha
    in [0, 1] with exact zeros -> (norm, gt_norm, alpha) float32"""
    rng = np.random.RandomState(2000 * seed + 3 * H + W)
    n = rng.randn(3, H, W)
    n /= np.linalg.norm(n, axis=0, keepdims=True)
    t = np.cross(n, rng.randn(3, H, W), axis=0)
    t /= np.linalg.norm(t, axis=0, keepdims=True)
    ang = np.radians(min_deg + (max_deg - min_deg) * rng.rand(H, W))
    m = np.cos(ang) * n + np.sin(ang) * t
    scale = 0.5 + rng.rand(1, H, W)          # not unit length: the division by the norms matters
    alpha = np.clip(1.5 * rng.rand(1, H, W) - 0.25, 0.0, 1.0)
    return (np.ascontiguousarray(n, np.float32), np.ascontiguousarray(m * scale, np.float32),
            np.ascontiguousarray(alpha, np.float32))


_GOLD = []


def golden():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")))
    return _GOLD[0]
