"""Make tests/golden/ingest.npz on a CPU: what the installed Pillow and the reference's own lines (in CPU torch) return for the inputs
of tests/ingest_ref.py.  Needs Pillow; the tests that read the file need neither Pillow nor the reference.

    python tests/golden/make_ingest_golden.py [--reference DIR]

With --reference DIR, `PILtoTorch` is imported from DIR/utils/general.py (the reference checkout); without it, its three lines are
restated below.  The inputs are not stored: tests/ingest_ref.py makes them from an integer mix."""
import importlib.util
import os
import sys

import numpy as np
import torch
from PIL import Image
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ingest_ref as R  # noqa: E402

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX}


def _pil_to_torch_restated(pil_image, resolution):        # utils/general.py:21-27
    resized = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return resized.permute(2, 0, 1) if len(resized.shape) == 3 else resized.unsqueeze(dim=-1).permute(2, 0, 1)


def load_pil_to_torch(argv):
    if "--reference" not in argv:
        return _pil_to_torch_restated, "restated"
    path = os.path.join(argv[argv.index("--reference") + 1], "utils", "general.py")
    spec = importlib.util.spec_from_file_location("reference_general", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PILtoTorch, "reference"


def camera_lines(pil_to_torch, image, alpha, normal, resolution):
    """utils/cameras.py:103-122 and Camera.__init__ :44-54, on the CPU"""
    rgb = pil_to_torch(image, resolution)
    a = pil_to_torch(alpha, resolution) if alpha is not None else None
    n = pil_to_torch(normal, resolution) if normal is not None else None
    gt_image = rgb[:3, ...]
    mask = (a[0:1, ...] > 0).float() if a is not None else None
    gt_normal = n[:3, ...] * 2. - 1. if n is not None else None
    original = gt_image.clamp(0.0, 1.0)
    if mask is not None:
        original *= mask
    else:
        original *= torch.ones((1, original.shape[1], original.shape[2]))
    return original, mask, gt_normal


def main(argv):
    pil_to_torch, source = load_pil_to_torch(argv)
    out = {"pillow_version": np.array(PIL.__version__), "pil_to_torch_source": np.array(source)}
    for shape, size in R.HOST_CASES:
        for kind in R.KINDS:
            img = R.noise(shape, R.case_seed(shape, size), kind)
            for name in R.FILTERS:
                out[R.case_key(shape, size, name, kind)] = np.array(Image.fromarray(img).resize(size, PIL_FILTER[name]))
    # Image.resize without a filter, as the reference calls it, through PILtoTorch
    for shape, size in R.P2T_CASES:
        img = R.noise(shape, R.case_seed(shape, size), "noise")
        t = pil_to_torch(Image.fromarray(img), size)
        assert t.dtype == torch.float32
        out["p2t_" + R.case_key(shape, size, "default", "noise")] = t.contiguous().numpy()
    for name, (H, W), res, with_alpha, with_normal in R.CAMERA_CASES:
        image, alpha, normal = R.camera_inputs(H, W)
        o, m, n = camera_lines(pil_to_torch, Image.fromarray(image), Image.fromarray(alpha) if with_alpha else None,
                               Image.fromarray(normal) if with_normal else None, res)
        out[f"cam_{name}_original"] = o.contiguous().numpy()
        if m is not None:
            out[f"cam_{name}_mask"] = m.contiguous().numpy()
        if n is not None:
            out[f"cam_{name}_normal"] = n.contiguous().numpy()
    rgba = R.composite_input()
    for tag, bg in (("bg0", [0, 0, 0]), ("bg1", [1, 1, 1])):           # dataset/dataset_readers.py:219-225
        norm_data = rgba / 255.0
        arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + np.array(bg) * (1 - norm_data[:, :, 3:4])
        # (Image.fromarray(..., "RGB") reads the int8 array's bytes; the installed Pillow wants them typed uint8)
        out["composite_" + tag] = np.array(Image.fromarray(np.array(arr * 255.0, dtype=np.byte).view(np.uint8), "RGB"))
    path = os.path.join(HERE, "ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries, PILtoTorch:", source)


if __name__ == "__main__":
    main(sys.argv[1:])
