"""Drop-in for the part of the `lpips` package that Texture-GS calls (utils/metrics.py:14,49-58 of the reference):

    from lpips import LPIPS
    LPIPS(net="vgg").to(device)(img1, img2, normalize=True).item()

With texture-gs_amd/ on PYTHONPATH this is texgs.lpips.LPIPSVGG -- thirteen HIP convolutions on the matrix cores and a HIP head --
so the reference's `utils/metrics.py` imports and runs as written, without the lpips package and without torchvision.

Weights are never downloaded.  They are looked for in this order:
    lin weights (the package's lpips/weights/v0.1/vgg.pth)     `model_path=`, else $TEXGS_LPIPS_LIN
    VGG16 (torchvision's vgg16-397923af.pth)                   `vgg_path=`, else $TEXGS_LPIPS_VGG, else that file under
                                                               torch.hub.get_dir()/checkpoints
and a FileNotFoundError names both files and both variables when one is missing.

Only `net="vgg"`, version 0.1, the scalar metric: `net="alex"` / `"squeeze"`, `spatial=True`, `lpips=False`, `pretrained=False`
and `retPerLayer=True` raise NotImplementedError by name.  The architecture is restated from the package's published source and is
UNPINNED (texgs.lpips says so in a RuntimeWarning).  As in the package, the value is differentiable in the two images -- with grad
mode on and an input that requires grad, `backward()` fills its `.grad` (texgs/lpips_grad.py; once per forward, no double backward,
the weights are constants).  There is no CPU fallback."""
import os

import torch

from texgs import lpips as _lpips

__all__ = ["LPIPS"]

VGG_FILE = "vgg16-397923af.pth"
LIN_FILE = "vgg.pth"


def _find_weights(model_path, vgg_path):
    lin = model_path or os.environ.get("TEXGS_LPIPS_LIN")
    vgg = vgg_path or os.environ.get("TEXGS_LPIPS_VGG") or os.path.join(torch.hub.get_dir(), "checkpoints", VGG_FILE)
    missing = [str(p) for p in (lin, vgg) if not p or not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(
            f"lpips drop-in: weight file(s) not found ({', '.join(missing)}).  It needs the lpips package's lin weights {LIN_FILE} "
            f"(model_path= or $TEXGS_LPIPS_LIN) and torchvision's {VGG_FILE} (vgg_path=, $TEXGS_LPIPS_VGG, or "
            f"{os.path.join(torch.hub.get_dir(), 'checkpoints')}); nothing is downloaded")
    return lin, vgg


class LPIPS(_lpips.LPIPSVGG):
    """lpips.LPIPS(net="vgg"): `.to()`, `.eval()` and `.cuda()` return self; calling it returns f32 [P,1,1,1] on the device."""

    def __init__(self, pretrained=True, net="alex", version="0.1", lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=True, vgg_path=None, precision="fp32"):
        if net != "vgg":
            raise NotImplementedError(f"lpips drop-in: net={net!r} is not supported (only net='vgg')")
        if spatial:
            raise NotImplementedError("lpips drop-in: spatial=True is not supported (the scalar metric only)")
        if not lpips:
            raise NotImplementedError("lpips drop-in: lpips=False (no lin layers) is not supported")
        if not pretrained:
            raise NotImplementedError("lpips drop-in: pretrained=False is not supported (the lin weights come from a file)")
        if str(version) != "0.1":
            raise NotImplementedError(f"lpips drop-in: version={version!r} is not supported (only '0.1')")
        if pnet_rand:
            raise NotImplementedError("lpips drop-in: pnet_rand=True is not supported (the VGG weights come from a file)")
        lin, vgg = _find_weights(model_path, vgg_path)
        super().__init__(vgg, lin, precision=precision)

    def __call__(self, in0, in1, retPerLayer=False, normalize=False):
        if retPerLayer:
            raise NotImplementedError("lpips drop-in: retPerLayer=True is not supported (texgs.lpips.LPIPSVGG.layers has the terms)")
        return super().__call__(in0, in1, normalize=normalize)

    forward = __call__
