#!/usr/bin/env python3
"""The evaluation of one view (train.py:45-93) two ways, timed in the same process at 800x800 and 1600x1200:

  hip        texgs.metrics.Evaluator.add(image, gt): one launch of csrc/metrics.hip plus its one-block reduce, nothing read back.
             add_ms          one call between a pair of device events after a synchronise: latency on an idle queue, launch gaps included
             add_batched_ms  --batch calls between one pair of events, divided by their number: device work per call
             The same two figures with normals and alpha (`*_normals_*`).
  reference  what the reference runs per view on clamped device images: l1_loss(...).mean().item(), psnr(...).mean().item() (torch
             float32, two readbacks), then both images copied to the host and the 7x7 SSIM there.  skimage is not installed where
             this project is developed, so the host SSIM is tests/metrics_ref.py (the same scipy.ndimage.uniform_filter calls, in
             float64 where skimage stays in float32); host wall clock, each leg ending in its readback.  Without scipy the host leg
             is omitted and the row says so.

Next to them: the kernel's achieved input bytes per second (2 x 3 x H x W x 4 bytes over add_batched_ms) and, measured the same way in
the same run, a device-to-device copy of a buffer of exactly that many bytes.  The images are seeded noise; calls run back to back, so
a 7.7 MB (800x800) or 23 MB (1600x1200) pair stays in the 256 MB Infinity Cache: the rates are not HBM rates.

Writes profiles/metrics_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_metrics.py [--iters 200] [--batch 20] [--warmup 20] [--ref-iters 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import metrics  # noqa: E402

try:
    import scipy.ndimage  # noqa: F401
    import metrics_ref
    HAVE_SCIPY = True
except ImportError:
    HAVE_SCIPY = False


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def batch_ms(f, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(k):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def ref_device_leg(image, gt):
    """l1_loss(...).mean().item() and psnr(...).mean().item() as train.py:67,69 call them"""
    l1 = torch.abs(image - gt).mean().mean().item()
    mse = ((image - gt) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
    return l1, (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().item()


def ref_host_leg(image, gt):
    """utils/metrics.py:40-46 with the statement in skimage's place"""
    return metrics_ref.ssim(image.detach().cpu().numpy(), gt.detach().cpu().numpy())


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed single calls of each HIP variant per row (at least 20)")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ref-iters", type=int, default=20, help="timed runs of the reference's pattern per row")
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 800, 1200, 1600], help="H W pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    rows = []
    for H, W in zip(args.sizes[0::2], args.sizes[1::2]):
        g = torch.Generator().manual_seed(H + W)
        image = (1.2 * torch.rand(3, H, W, generator=g) - 0.1).to(dev)
        gt = torch.rand(3, H, W, generator=g).to(dev)
        norm, gt_norm = torch.randn(3, H, W, generator=g).to(dev), torch.randn(3, H, W, generator=g).to(dev)
        alpha = torch.rand(1, H, W, generator=g).to(dev)
        in_bytes = 2 * 3 * H * W * 4
        src = torch.empty(in_bytes // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        cap = 2 * (args.warmup + args.iters + (args.iters // args.batch + 1) * args.batch) + 8
        ev = metrics.Evaluator(capacity=cap)
        rgb = lambda: ev.add(image, gt)                                               # noqa: E731
        full = lambda: ev.add(image, gt, norm=norm, gt_norm=gt_norm, alpha=alpha)     # noqa: E731
        copy = lambda: dst.copy_(src)                                                 # noqa: E731
        for _ in range(args.warmup):
            rgb(), full(), copy()
        t_rgb, t_full, t_copy = [], [], []
        for _ in range(args.iters):                     # alternating
            t_rgb.append(event_ms(rgb))
            t_full.append(event_ms(full))
            t_copy.append(event_ms(copy))
        b_rgb, b_full, b_copy = [], [], []
        for _ in range(max(1, args.iters // args.batch)):
            b_rgb.append(batch_ms(rgb, args.batch))
            b_full.append(batch_ms(full, args.batch))
            b_copy.append(batch_ms(copy, args.batch))
        res = ev.result()
        row = {"H": H, "W": W, "input_mb": round(in_bytes / 1e6, 2), "add_ms": med(t_rgb), "add_batched_ms": med(b_rgb),
               "add_p10_p90_ms": [round(float(np.percentile(t_rgb, q)), 4) for q in (10, 90)],
               "add_normals_ms": med(t_full), "add_normals_batched_ms": med(b_full),
               "copy_ms": med(t_copy), "copy_batched_ms": med(b_copy)}
        row["kernel_input_gbps"] = round(in_bytes / (row["add_batched_ms"] * 1e-3) / 1e9, 1)
        row["copy_read_gbps"] = round(in_bytes / (row["copy_batched_ms"] * 1e-3) / 1e9, 1)
        ic, gc = torch.clamp(image, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)
        for _ in range(3):
            ref_device_leg(ic, gc)
        t_dev, t_host = [], []
        for _ in range(args.ref_iters):
            t_dev.append(wall_ms(lambda: ref_device_leg(ic, gc))[0])
            if HAVE_SCIPY:
                ms, ref_ssim = wall_ms(lambda: ref_host_leg(ic, gc))
                t_host.append(ms)
        row["reference_l1_psnr_item_ms"] = med(t_dev)
        if HAVE_SCIPY:
            row["reference_host_ssim_ms"] = med(t_host)
            row["reference_view_ms"] = round(row["reference_l1_psnr_item_ms"] + row["reference_host_ssim_ms"], 4)
            row["reference_over_add"] = round(row["reference_view_ms"] / row["add_ms"], 1)
            row["ssim_difference_from_host"] = abs(ref_ssim - res["ssim"])
        else:
            row["reference_host_ssim_ms"] = None
            row["note"] = "scipy is not importable: the host SSIM leg is omitted"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ev, image, gt, norm, gt_norm, alpha, src, dst
        torch.cuda.empty_cache()
    out = {"metric": "Evaluator.add against the reference's per-view pattern; device-event ms (median): add_ms = one call on an idle "
                     "queue, launch gaps included; *_batched_ms = per call with --batch calls between one event pair; reference_* = "
                     "host wall clock, each leg ending in its readback; *_gbps = input bytes over the batched time, copy_* a "
                     "device-to-device copy of as many bytes (inputs stay in the Infinity Cache between calls)",
           "device": torch.cuda.get_device_name(0), "iters": args.iters, "batch": args.batch, "warmup": args.warmup,
           "ref_iters": args.ref_iters, "host_ssim": "tests/metrics_ref.py (scipy, float64)" if HAVE_SCIPY else None, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
