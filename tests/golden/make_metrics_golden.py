"""Generate tests/golden/metrics.npz: small views and the 16-value rows that tests/metrics_ref.py (the float64 numpy / scipy
statement of the evaluation metrics) gives for them.  Needs scipy, not the reference tree: skimage is not installed where this
project is developed, so the rows pin the STATEMENT (and through it the kernel), not skimage's output.

  <tag>_image, _gt, [_norm, _gt_norm, [_alpha]], _clamp, _row        tags: noise9x11, range12x10, smooth33x35

Usage: python tests/golden/make_metrics_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as M  # noqa: E402

CASES = [("noise9x11", "noise", 9, 11, False, False, False),
         ("range12x10", "out_of_range", 12, 10, True, True, True),
         ("smooth33x35", "smooth", 33, 35, True, True, False)]


def main():
    rec = {}
    for tag, kind, H, W, clamp, normals, with_alpha in CASES:
        image, gt = M.image_pair(kind, H, W, seed=5)
        norm = gt_norm = alpha = None
        if normals:
            norm, gt_norm, alpha = M.normal_pair(H, W, seed=5)
            if not with_alpha:
                alpha = None
        rec[f"{tag}_image"], rec[f"{tag}_gt"], rec[f"{tag}_clamp"] = image, gt, np.array(clamp)
        for k, v in (("norm", norm), ("gt_norm", gt_norm), ("alpha", alpha)):
            if v is not None:
                rec[f"{tag}_{k}"] = v
        rec[f"{tag}_row"] = M.row(image, gt, norm, gt_norm, alpha, clamp=clamp)
    assert (rec["range12x10_image"] > 1).any() and (rec["range12x10_image"] < 0).any() and (rec["range12x10_alpha"] == 0).any()
    out = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
