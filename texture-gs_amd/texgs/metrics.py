"""Evaluation metrics (train.py:45-93 `visualize`, utils/metrics.py) on the device: L1, PSNR, SSIM and the normal MAE of a view from
ONE launch of csrc/metrics.hip, which leaves every sum the four need in a row of 16 float64 values (include/texgs.h
TEXGS_METRICS_*).  The reference copies both images to the host for skimage's SSIM and reads three scalars back per view; here
`Evaluator.add` enqueues and returns, and `Evaluator.result` reads the whole table back once.

`mse`, `psnr`, `ssim`, `mae` and `avg_error` keep the reference's signatures and return types.  SSIM is
skimage.metrics.structural_similarity(channel_axis=0, data_range=1.0) -- uniform 7x7 window, sample covariance, border of 3 cropped
-- NOT the training loss of texgs.losses (11x11 Gaussian window, zero padding, population covariance).  Images are float32 [3,H,W]
with H, W >= 7 (the window has to fit; skimage raises too), contiguous, on the GPU: there is no CPU fallback.

LPIPS-VGG is texgs.lpips (thirteen MFMA convolutions and a head in csrc/lpips.hip): `lpips(img1, img2, net)` below keeps the
reference's signature, `Evaluator(capacity, lpips=net)` adds its column.  Its network weights are not part of this project: the
user builds the net from the two published state dicts (texgs.lpips.LPIPSVGG).  The depth picture of train.py:22-37 is texgs.present.depth_colour;
OpenCV's own JET table comes in through its `lut=` argument."""
import numpy as np
import torch

from . import _lib
from .losses import _check_count, _check_device

ROW = _lib.METRICS_ROW


def _check_map(name, t, channels, H, W):
    _check_count(name, t, channels, H, W)
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_view(image, gt_image, norm, gt_norm, alpha):
    """Everything a launch relies on, before any library call -> (H, W, alpha as float32 or None)"""
    if not torch.is_tensor(image) or not torch.is_tensor(gt_image) or image.dim() != 3 or image.shape[0] != 3 \
            or gt_image.shape != image.shape:
        raise ValueError("image and gt_image must both be [3,H,W], got "
                         f"{tuple(getattr(image, 'shape', ()))} and {tuple(getattr(gt_image, 'shape', ()))}")
    _, H, W = image.shape
    if H < 7 or W < 7:
        raise ValueError(f"H and W must be at least 7 (the 7x7 SSIM window has to fit), got {H}x{W}")
    _check_map("image", image, 3, H, W)
    _check_map("gt_image", gt_image, 3, H, W)
    if (norm is None) != (gt_norm is None):
        raise ValueError("norm and gt_norm must be given together")
    if norm is not None:
        for name, t in (("norm", norm), ("gt_norm", gt_norm)):
            if not torch.is_tensor(t) or t.dim() != 3 or tuple(t.shape) != (3, H, W):
                raise ValueError(f"{name} must be [3,{H},{W}], got {tuple(getattr(t, 'shape', ()))}")
            _check_map(name, t, 3, H, W)
    if alpha is not None:
        if norm is None:
            raise ValueError("alpha weights the normal MAE: it needs norm and gt_norm")
        if not torch.is_tensor(alpha):
            raise ValueError("alpha must be a tensor of H W elements")
        _check_count("alpha", alpha, 1, H, W)
        if not alpha.is_contiguous():
            raise ValueError("alpha must be contiguous")
    if image.device.type != "cuda":
        raise RuntimeError("texgs.metrics runs on an AMD GPU; there is no CPU fallback")
    _check_device(image.device, gt_image=gt_image, norm=norm, gt_norm=gt_norm, alpha=alpha)
    if alpha is not None:
        alpha = alpha.float()           # (the reference's `alpha.float()`: a bool mask is converted on the device)
    return H, W, alpha


def _launch(image, gt_image, norm, gt_norm, alpha, H, W, clamp, table, v):
    """Enqueue the view's kernels on the current stream; they write row v of `table` (f64 [capacity, 16])"""
    lib = _lib.load()
    dev = image.device
    temp = torch.empty(lib.texgs_eval_metrics_temp_bytes(H, W) // 8, dtype=torch.float64, device=dev)
    p = _lib.ptr
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_eval_metrics, p(image), p(gt_image), p(norm), p(gt_norm), p(alpha), H, W, 1 if clamp else 0, p(temp),
                  table.data_ptr() + v * ROW * 8, stream)


def _det(*ts):
    return tuple(t.detach() if torch.is_tensor(t) else t for t in ts)     # (anything else is refused by _check_view)


def _row(image, gt_image, norm=None, gt_norm=None, alpha=None, clamp=False):
    """One view's row as a device tensor f64[16]"""
    image, gt_image, norm, gt_norm, alpha = _det(image, gt_image, norm, gt_norm, alpha)
    H, W, alpha = _check_view(image, gt_image, norm, gt_norm, alpha)
    table = torch.empty(1, ROW, dtype=torch.float64, device=image.device)
    _launch(image, gt_image, norm, gt_norm, alpha, H, W, clamp, table, 0)
    return table[0]


def mse(img1, img2):
    """utils/metrics.py:18-19: per-channel mean squared error, a [3,1] float32 tensor on the device (nothing is read back)"""
    r = _row(img1, img2)
    return (r[1:4] / r[9]).to(torch.float32).view(3, 1)


def psnr(img1, img2):
    """utils/metrics.py:21-23: 20 log10(1 / sqrt(mse)) per channel, [3,1] float32 on the device; an identical pair gives inf"""
    r = _row(img1, img2)
    return (20.0 * torch.log10(1.0 / torch.sqrt(r[1:4] / r[9]))).to(torch.float32).view(3, 1)


def ssim(img1, img2):
    """utils/metrics.py:40-46: the mean over channels of skimage's mean SSIM, a Python float.  One readback of three sums; the
    images stay on the device."""
    r = _row(img1, img2)[4:11].cpu().numpy()
    return float(np.mean(r[0:3] / r[6]))


def mae(norm1, norm2, alpha=None):
    """utils/metrics.py:25-37: mean angle between two normal maps in degrees, weighted by alpha when given; a 0-d float32 tensor on
    the device.  NaN when alpha sums to zero, as in the reference.  (The kernel works on a view: the normals stand in for its image
    pair, whose sums are not used.)"""
    r = _row(norm1, norm2, norm1, norm2, alpha)
    return (r[7] / r[8]).to(torch.float32)


_default_lpips = None


def set_lpips(net):
    """Install the module default that `lpips(img1, img2)` uses: a texgs.lpips.LPIPSVGG, or None to remove it"""
    global _default_lpips
    _default_lpips = net


def lpips(img1, img2, net=None):
    """utils/metrics.py:49-58: LPIPS-VGG of ONE pair of [3,H,W] (or [1,3,H,W]) images in [0,1] (`normalize=True`), a Python float
    from one readback.  `net`: a texgs.lpips.LPIPSVGG, else the default installed with `set_lpips`.  Several pairs have no single
    float: they are refused by name (call the net itself for a [P,1,1,1] tensor)."""
    net = _default_lpips if net is None else net
    if net is None:
        raise RuntimeError("no LPIPS network: build one with texgs.lpips.LPIPSVGG(vgg_state, lin_state) -- torchvision's VGG16 state "
                           "dict and the lpips package's vgg.pth -- and pass it as net= or install it with texgs.metrics.set_lpips(net)")
    for name, t in (("img1", img1), ("img2", img2)):
        if torch.is_tensor(t) and t.dim() == 4 and t.shape[0] != 1:
            raise ValueError(f"metrics.lpips returns one float for one pair; {name} holds {t.shape[0]} images: call net(img1, img2, "
                             "normalize=True) for a [P,1,1,1] tensor")
    with torch.no_grad():               # a metric: never the differentiable path, whatever the images require
        return net(img1, img2, normalize=True).item()


def avg_error(psnr, ssim, lpips):
    """The 'average' error used in the paper (utils/metrics.py:60-67), host arithmetic."""
    def psnr_to_mse(psnr):
        return np.exp(-0.1 * np.log(10.) * psnr)
    mse = psnr_to_mse(psnr)
    dssim = np.sqrt(1 - ssim)
    return np.exp(np.mean(np.log(np.array([mse, dssim, lpips])))).item()


def finish_rows(rows, has_norm):
    """The host half of `Evaluator.result`: rows float64 [V, 16] as the kernel wrote them, has_norm one bool per view ->
    dict(views, l1, psnr, ssim, mae), float64 arithmetic.  l1, psnr and ssim are means over views of the per-view values as
    train.py:67-69,90-92 average them (PSNR per channel, then over channels, then over views); mae is the mean over the views that
    had normals of their (alpha-weighted) mean angle in degrees, None when no view had any."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    V = rows.shape[0]
    has_norm = np.asarray(has_norm, dtype=bool).reshape(-1)
    if has_norm.shape[0] != V:
        raise ValueError(f"has_norm holds {has_norm.shape[0]} entries for {V} rows")
    if V == 0:
        return dict(views=0, l1=None, psnr=None, ssim=None, mae=None)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = rows[:, 0] / (3.0 * rows[:, 9])
        ps = (20.0 * np.log10(1.0 / np.sqrt(rows[:, 1:4] / rows[:, 9:10]))).mean(axis=1)
        ss = (rows[:, 4:7] / rows[:, 10:11]).mean(axis=1)
        ma = rows[has_norm, 7] / rows[has_norm, 8]
    return dict(views=V, l1=float(l1.mean()), psnr=float(ps.mean()), ssim=float(ss.mean()),
                mae=float(ma.mean()) if ma.size else None)


class Evaluator:
    """The evaluation loop of train.py:45-93 without its per-view readbacks:

        ev = Evaluator(capacity=len(cameras))
        for view in cameras:
            ev.add(image, gt_image, norm=norm, gt_norm=gt_normal, alpha=gt_alpha)     # enqueues; synchronises nothing
        res = ev.result()                                                             # one readback

    `clamp=True` clamps image and gt_image to [0, 1] in the kernel (train.py:52,58); normals and alpha are never clamped.

    `Evaluator(capacity, lpips=net)` with a texgs.lpips.LPIPSVGG: `add` also enqueues the LPIPS (`normalize=True`) of the pair --
    clamped when `clamp` -- into a second device table, still without synchronising anything; `result` reads that table in the same
    call and adds "lpips" (the mean over views) and "avg_error" (of the three means).  Without it nothing changes."""

    def __init__(self, capacity, lpips=None):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.capacity = capacity
        self._table = None          # f64 [capacity, 16] on the device of the first view
        self._has_norm = []
        self._lpips = lpips
        self._lpips_table = None    # f64 [capacity, 8] (texgs.lpips.ROW) next to it

    def __len__(self):
        return len(self._has_norm)

    def add(self, image, gt_image, norm=None, gt_norm=None, alpha=None, clamp=True):
        image, gt_image, norm, gt_norm, alpha = _det(image, gt_image, norm, gt_norm, alpha)
        H, W, alpha = _check_view(image, gt_image, norm, gt_norm, alpha)
        v = len(self._has_norm)
        if v >= self.capacity:
            raise RuntimeError(f"the evaluator holds {self.capacity} views already (its capacity)")
        if self._table is None:
            self._table = torch.zeros(self.capacity, ROW, dtype=torch.float64, device=image.device)
        elif self._table.device != image.device:
            raise ValueError(f"image is on {image.device}, the earlier views were on {self._table.device}")
        _launch(image, gt_image, norm, gt_norm, alpha, H, W, clamp, self._table, v)
        if self._lpips is not None:
            if self._lpips_table is None:
                from .lpips import ROW as LPIPS_ROW
                self._lpips_table = torch.zeros(self.capacity, LPIPS_ROW, dtype=torch.float64, device=image.device)
            a, b = (image.clamp(0.0, 1.0), gt_image.clamp(0.0, 1.0)) if clamp else (image, gt_image)
            self._lpips.table(a, b, normalize=True, out=self._lpips_table[v:v + 1])
        self._has_norm.append(norm is not None)

    def rows(self):
        """The raw table of the views added so far, float64 [views, 16] on the device"""
        v = len(self._has_norm)
        if self._table is None:
            return torch.zeros(0, ROW, dtype=torch.float64)
        return self._table[:v]

    def result(self):
        rows = self.rows()
        if self._lpips is None:
            return finish_rows(rows.cpu().numpy(), self._has_norm)
        v = len(self._has_norm)
        if v == 0:
            return dict(finish_rows(rows.cpu().numpy(), self._has_norm), lpips=None, avg_error=None)
        from .lpips import LAYERS
        both = torch.cat([rows, self._lpips_table[:v]], dim=1).cpu().numpy()          # one readback
        res = finish_rows(both[:, :ROW], self._has_norm)
        res["lpips"] = float(both[:, ROW + LAYERS].mean())
        res["avg_error"] = avg_error(res["psnr"], res["ssim"], res["lpips"])
        return res
