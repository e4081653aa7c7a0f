#!/usr/bin/env python3
"""How much of the cloud the 3-NN search of csrc/points.hip visits, from a debug build of the library with its counters compiled in:

  TEXGS_EXTRA_FLAGS=-DTEXGS_POINTS_STATS TEXGS_LIB_NAME=libtexgs_stats.so TEXGS_OBJ_DIR=build_stats python texture-gs_amd/build.py
  TEXGS_LIB=texture-gs_amd/libtexgs_stats.so python scripts/points_box_stats.py [--out profiles/points_box_stats.json]

Per cloud of scripts/bench_points.py: boxes (of 256 points) in the cloud, candidate boxes staged in LDS per query box, and boxes a
query point scans itself on average.  The shipped library has no counters."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import _lib, points  # noqa: E402
import bench_points as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_box_stats.json"))
    args = ap.parse_args()
    lib = _lib.load()
    if not hasattr(lib, "texgs_points_stats"):
        raise SystemExit("this library has no counters: build it with -DTEXGS_POINTS_STATS (see the docstring)")
    lib.texgs_points_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    rows = []
    for n in (100_000, 300_000, 1_000_000):
        for cloud in ("uniform", "clustered"):
            x = torch.from_numpy(getattr(B, cloud)(n, 1)).cuda()
            assert lib.texgs_points_stats(None, 1) == 0
            points.knn3_mean_dist2(x)
            st = (C.c_ulonglong * 4)()
            assert lib.texgs_points_stats(st, 1) == 0
            qboxes, staged, scans, qpoints = (int(v) for v in st)
            rows.append({"N": n, "cloud": cloud, "boxes": qboxes, "boxes_staged_per_query_box": round(staged / qboxes, 2),
                         "boxes_scanned_per_point": round(scans / qpoints, 2)})
            print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
