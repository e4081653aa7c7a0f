#!/usr/bin/env python3
"""Kernel times of the output stage (csrc/present.hip) from a rocprofv3 kernel trace, per shape.

scripts/bench_present.py times CALLS: at these frame sizes a call is bounded by its enqueue (a few microseconds of Python and ctypes),
not by the kernel, so its batched figure says little about the kernel.  This script has two halves:

  run    launch each kernel --count times per shape in a fixed order (to be run under the profiler, in a run of its own):
             rocprofv3 --kernel-trace -d DIR -o present -- python scripts/present_kernel_times.py run
  parse  read DIR's *_results.db (or, with --output-format csv, its *_kernel_trace.csv), cut the dispatches of k_present /
         k_depth_range / k_depth_colour / k_cube_cross into that same order, and write per shape the median kernel time, the algorithmic bytes from the shapes and their quotient:
             python scripts/present_kernel_times.py parse DIR/present_results.db [--out profiles/present_kernel_times.json]

Every launch re-reads the same buffers, so frames of these sizes come from the 256 MB Infinity Cache, not from HBM (the R = 2048
texture, 302 MB, does not fit)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(800, 800), (1200, 1600)]
CROSS = [1024, 2048]
KERNELS = ("k_present", "k_depth_range", "k_depth_colour", "k_cube_cross")


def plan(count):
    """[(label, shape, {kernel: (launches, algorithmic bytes per launch)})] in launch order"""
    steps = []
    for H, W in SIZES:
        P = H * W
        steps.append(("frame_u8 composite", {"H": H, "W": W}, {"k_present": (count, P * (12 + 4 + 3))}))
        steps.append(("depth_colour masked, f32 planes out", {"H": H, "W": W},
                      {"k_depth_range": (count, P * 8), "k_depth_colour": (count, P * (8 + 12))}))
        steps.append(("display rgb", {"H": H, "W": W}, {"k_present": (count, P * (12 + 16))}))
    for R in CROSS:
        steps.append(("cross_u8", {"R": R}, {"k_cube_cross": (count, 6 * R * R * 12 + 12 * R * R * 3)}))
    return steps


def run(count):
    import warnings
    import torch
    from texgs import present
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda:0")
    lut = present.jet_lut(dev)
    for H, W in SIZES:
        g = torch.Generator().manual_seed(H + W)
        image = (1.4 * torch.rand(3, H, W, generator=g) - 0.2).to(dev)
        alpha = (torch.rand(1, H, W, generator=g) > 0.3).float().to(dev)
        depth = (0.5 + 6 * torch.rand(1, H, W, generator=g)).to(dev)
        bg = torch.tensor([0.1, 0.7, 0.33], device=dev)
        out_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        out4 = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
        for _ in range(count):
            present.frame_u8(image, alpha=alpha, background=bg, out=out_u8)
        for _ in range(count):
            present.depth_colour(depth, mask=alpha, lut=lut)
        for _ in range(count):
            present.display(image, out=out4)
        torch.cuda.synchronize()
    for R in CROSS:
        texture = (4.4 * torch.rand(6, R, R, 3, generator=torch.Generator().manual_seed(R)) - 2.2).to(dev)
        out = torch.empty(3 * R, 4 * R, 3, dtype=torch.uint8, device=dev)
        for _ in range(count):
            present.cross_u8(texture, out=out)
        torch.cuda.synchronize()
        del texture, out
    print(json.dumps({"launched": [(label, shape) for label, shape, _ in plan(count)], "count": count}))


def dispatches(path):
    """[(kernel name, start ns, end ns)] from the profiler's output: its sqlite database (the `kernels` view) or a kernel-trace csv"""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as db:
            return [(n, int(a), int(b)) for n, a, b in db.execute("select name, start, end from kernels")]
    with open(path, newline="") as f:
        return [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]


def parse(path, count, out):
    per = {k: [] for k in KERNELS}
    for name, start, end in sorted(dispatches(path), key=lambda r: r[1]):
        for k in KERNELS:
            if k + "(" in name or name.endswith(k):
                per[k].append((end - start) / 1e3)      # microseconds
    result = []
    for label, shape, kernels in plan(count):
        for k, (n, nbytes) in kernels.items():
            if len(per[k]) < n:
                raise SystemExit(f"the trace holds too few dispatches of {k}: was it recorded with --count {count}?")
            us, per[k] = per[k][:n], per[k][n:]
            us = us[n // 5:]                    # the first fifth warms the caches
            m = float(np.median(us))
            result.append({"call": label, **shape, "kernel": k, "launches": n, "kernel_us": round(m, 2),
                           "kernel_us_p10_p90": [round(float(np.percentile(us, q)), 2) for q in (10, 90)],
                           "algorithmic_mb": round(nbytes / 1e6, 2), "algorithmic_gbps": round(nbytes / (m * 1e-6) / 1e9, 1)})
    left = {k: len(v) for k, v in per.items() if v}
    if left:
        raise SystemExit(f"dispatches left over after the plan: {left}")
    doc = {"metric": "rocprofv3 --kernel-trace, End - Start per dispatch, median over the launches of one shape after the first fifth; "
                     "algorithmic bytes = inputs read once plus outputs written once, from the shapes.  Back-to-back launches on the "
                     "same buffers: frames of these sizes are served by the Infinity Cache, not by HBM.",
           "count": count, "rows": result}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in result:
        print(json.dumps(r))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "parse"])
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--count", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_kernel_times.json"))
    a = ap.parse_args()
    if a.mode == "run":
        run(a.count)
    else:
        if not a.trace:
            ap.error("parse needs the path of the profiler's database or kernel trace csv")
        parse(a.trace, a.count, a.out)
