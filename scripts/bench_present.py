#!/usr/bin/env python3
"""The output stage two ways, timed in the same process: the reference's own lines (torch launches, host waits, numpy on one core)
against texgs.present (one HIP pass, 8 bits over PCIe).  Rows, at 800x800 and 1600x1200 unless said otherwise:

  retexture   retexture.py:28-32 ending with the host uint8 array, against frame_u8 plus a pinned non-blocking readback ending the same way
  reader      32 frames through that reference loop against 32 frames through FrameReader(4), as frames per second
  depth       train.py:22-37 ending with the f32 [3,H,W] picture on the device, against depth_colour.  OpenCV is not installed where this
              project is developed: np.take on the table stands in for convertScaleAbs + applyColorMap + cvtColor (it does less work
              than they do, so the reference leg is flattered)
  viewer      viewer_renderer.py:138-173 (rgb mode) ending with the contiguous [H,W,4] frame, against display
  cross       cube_map plus extract_texture.py:17 at R = 1024 and 2048 ending with the host uint8 cross, against cross_u8 plus a pinned
              readback

Every leg is host wall clock around a call that ends synchronised, legs alternating inside one loop; medians, and the p10-p90 spread
of the reference leg.  verdict: "faster" / "slower" when the medians differ by more than that spread, "tie" inside it.  max_difference_from_reference is
the largest difference between the two legs' results in this run (the reference leg runs torch's GPU kernels, whose scalar division
multiplies by a reciprocal: the bit-exact comparison is the test suite's, against the CPU statement).

Next to each fused call: its algorithmic bytes (inputs read once plus outputs written once, from the shapes) over its batched
device-event time (--batch calls between one event pair), and a device-to-device copy of a buffer of exactly that many bytes (read plus
written) measured the same way in the same run.  At these frame sizes a batched call is bounded by its ENQUEUE (Python, ctypes, the
launch), not by the kernel: call_gbps is a floor, and the kernels' own times come from the profiler (scripts/present_kernel_times.py,
profiles/present_kernel_times.json).  Calls run back to back on the same buffers, so a frame of these sizes stays in the 256 MB
Infinity Cache: none of these rates is an HBM rate (the R = 2048 cross, 302 MB in, is the exception).

Writes profiles/present_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_present.py [--reps 30] [--batch 20] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import present  # noqa: E402


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def batch_ms(f, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(k):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def med(v):
    return round(float(np.median(v)), 4)


def compare(ref, fused, warmup, reps):
    """Alternating wall-clock repetitions -> the row's timing fields"""
    for _ in range(warmup):
        ref(), fused()
    t_ref, t_fused = [], []
    for _ in range(reps):
        t_ref.append(wall_ms(ref))
        t_fused.append(wall_ms(fused))
    spread = float(np.percentile(t_ref, 90) - np.percentile(t_ref, 10))
    r, f = float(np.median(t_ref)), float(np.median(t_fused))
    verdict = "tie" if abs(r - f) <= spread else ("faster" if f < r else "slower")
    return {"reference_ms": round(r, 4), "fused_ms": round(f, 4), "reference_p10_p90_spread_ms": round(spread, 4),
            "fused_p10_p90_ms": [round(float(np.percentile(t_fused, q)), 4) for q in (10, 90)],
            "reference_over_fused": round(r / f, 2), "verdict": verdict}


def kernel_rate(f, nbytes, dev, batch, rounds=5):
    """The call's batched time, its algorithmic bytes per second, and a device copy moving as many bytes (half read, half written)"""
    src = torch.empty(max(1, nbytes // 2), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)           # noqa: E731
    f(), copy()
    k, c = [], []
    for _ in range(rounds):                 # alternating
        k.append(batch_ms(f, batch))
        c.append(batch_ms(copy, batch))
    km, cm = float(np.median(k)), float(np.median(c))
    return {"call_batched_ms": round(km, 4), "algorithmic_mb": round(nbytes / 1e6, 2), "call_gbps": round(nbytes / (km * 1e-3) / 1e9, 1),
            "copy_batched_ms": round(cm, 4), "copy_gbps": round(nbytes / (cm * 1e-3) / 1e9, 1)}


# ---- the reference's lines ----
def ref_retexture(image, gt_alpha, background):
    image = torch.clamp(image, 0.0, 1.0)
    image = image * gt_alpha.repeat(3, 1, 1) + background[:, None, None].expand_as(image) * (1 - gt_alpha.repeat(3, 1, 1))
    return (image.permute(1, 2, 0).detach().cpu().numpy() * 255).astype(np.uint8).copy()


def ref_depth(depth, mask, lut_np):
    depth = depth.squeeze(0)
    mask = mask.bool().squeeze(0)
    device = depth.device
    min_d, max_d = torch.min(depth[mask]), torch.max(depth[mask])
    depth = torch.clamp((depth - min_d) / (max_d - min_d + 1e-8), 0.0, 1.0)
    scaled = np.clip(np.rint(np.abs(depth.detach().cpu().numpy() * 255)), 0, 255).astype(np.uint8)      # convertScaleAbs
    d_color = torch.tensor(np.take(lut_np, scaled, axis=0), device=device)                              # applyColorMap + cvtColor
    d_color[~mask] = 0
    return (d_color.float() / 255).permute(2, 0, 1)


def ref_viewer(image):
    img = torch.clamp(image, 0.0, 1.0).permute(1, 2, 0)
    return torch.concat([img, torch.ones_like(img[..., :1])], dim=-1).contiguous()


def ref_cross(texture):
    rgb = torch.clamp(0.28209479177387814 * texture + 0.5, 0.0, 1.0)
    res = texture.shape[1]
    cubemap = torch.zeros((res * 3, res * 4, 3), dtype=rgb.dtype, device=rgb.device)
    cubemap[0:res, res:2 * res, :] = rgb[2]
    cubemap[res:2 * res, 0:res, :] = rgb[1]
    cubemap[res:2 * res, res:2 * res, :] = rgb[4]
    cubemap[res:2 * res, 2 * res:3 * res, :] = rgb[0]
    cubemap[res:2 * res, 3 * res:4 * res, :] = rgb[5]
    cubemap[2 * res:3 * res, res:2 * res, :] = rgb[3]
    return (torch.clamp(cubemap, 0, 1) * 255).detach().cpu().numpy().astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions per row")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 800, 1200, 1600], help="H W pairs")
    ap.add_argument("--cross", type=int, nargs="+", default=[1024, 2048], help="texture resolutions of the cross rows")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_present.py needs an MI355X: there is no CPU path to time")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda:0")
    lut_np = present.jet_table()
    lut = torch.from_numpy(lut_np).to(dev)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for H, W in zip(args.sizes[0::2], args.sizes[1::2]):
        g = torch.Generator().manual_seed(H + W)
        image = (1.4 * torch.rand(3, H, W, generator=g) - 0.2).to(dev)
        alpha = (torch.rand(1, H, W, generator=g) > 0.3).float().to(dev)
        depth = (0.5 + 6 * torch.rand(1, H, W, generator=g)).to(dev)
        bg = torch.tensor([0.1, 0.7, 0.33], device=dev)
        P = H * W
        shape = {"H": H, "W": W}
        # retexture
        out_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        pinned = torch.empty(H, W, 3, dtype=torch.uint8).pin_memory()

        def fused_retexture():
            present.frame_u8(image, alpha=alpha, background=bg, out=out_u8)
            pinned.copy_(out_u8, non_blocking=True)
            torch.cuda.synchronize()
            return pinned.numpy()
        differ = int(np.abs(fused_retexture().astype(np.int16) - ref_retexture(image, alpha, bg)).max())
        row = {"row": "retexture", **shape, "max_difference_from_reference": differ, **compare(lambda: ref_retexture(image, alpha, bg), fused_retexture, args.warmup, args.reps)}
        row.update(kernel_rate(lambda: present.frame_u8(image, alpha=alpha, background=bg, out=out_u8), P * (16 + 3), dev, args.batch))
        row["readback_mb"] = {"reference": round(P * 12 / 1e6, 2), "fused": round(P * 3 / 1e6, 2)}
        emit(row)
        # the reader
        reader = present.FrameReader(4, H, W)

        def ref_loop():
            return [ref_retexture(image, alpha, bg) for _ in range(args.frames)]

        def fused_loop():
            got = []
            for k in range(args.frames):
                got += reader.submit(k, image, alpha=alpha, background=bg)
            got += list(reader.drain())
            return got
        c = compare(ref_loop, fused_loop, 1, max(3, args.reps // 6))
        emit({"row": "reader", **shape, "frames": args.frames, "ring": 4, **c,
              "reference_fps": round(args.frames / (c["reference_ms"] * 1e-3), 1), "fused_fps": round(args.frames / (c["fused_ms"] * 1e-3), 1)})
        # depth
        row = {"row": "depth", **shape, "opencv": "np.take on the table stands in for convertScaleAbs + applyColorMap + cvtColor",
               **compare(lambda: ref_depth(depth, alpha, lut_np), lambda: present.depth_colour(depth, mask=alpha, lut=lut), args.warmup, args.reps)}
        row["max_difference_from_reference"] = float((ref_depth(depth, alpha, lut_np) - present.depth_colour(depth, mask=alpha, lut=lut)).abs().max())
        row.update(kernel_rate(lambda: present.depth_colour(depth, mask=alpha, lut=lut), P * (2 * 8 + 12), dev, args.batch))
        row["call_note"] = "two launches: depth and mask are read twice"
        emit(row)
        # viewer
        out4 = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
        differ = float((ref_viewer(image) - present.display(image)).abs().max())
        row = {"row": "viewer", **shape, "max_difference_from_reference": differ, **compare(lambda: ref_viewer(image), lambda: present.display(image, out=out4), args.warmup, args.reps)}
        row.update(kernel_rate(lambda: present.display(image, out=out4), P * (12 + 16), dev, args.batch))
        emit(row)
        del image, alpha, depth, out_u8, out4, pinned, reader
        torch.cuda.empty_cache()

    for R in args.cross:
        g = torch.Generator().manual_seed(R)
        texture = (4.4 * torch.rand(6, R, R, 3, generator=g) - 2.2).to(dev)
        out = torch.empty(3 * R, 4 * R, 3, dtype=torch.uint8, device=dev)
        pinned = torch.empty(3 * R, 4 * R, 3, dtype=torch.uint8).pin_memory()

        def fused_cross():
            present.cross_u8(texture, out=out)
            pinned.copy_(out, non_blocking=True)
            torch.cuda.synchronize()
            return pinned.numpy()
        differ = int(np.abs(fused_cross().astype(np.int16) - ref_cross(texture)).max())
        row = {"row": "cross", "R": R, "max_difference_from_reference": differ, **compare(lambda: ref_cross(texture), fused_cross, 1, max(3, args.reps // 6))}
        row.update(kernel_rate(lambda: present.cross_u8(texture, out=out), 6 * R * R * 12 + 12 * R * R * 3, dev, args.batch))
        row["readback_mb"] = {"reference": round(12 * R * R * 12 / 1e6, 1), "fused": round(12 * R * R * 3 / 1e6, 1)}
        emit(row)
        del texture, out, pinned
        torch.cuda.empty_cache()

    losers = [r for r in rows if r["verdict"] == "slower"]
    out = {"metric": "host wall-clock ms of a call that ends synchronised, medians of alternating repetitions in one process; verdict "
                     "against the reference leg's p10-p90 spread; call_batched_ms / call_gbps = device-event time per call with --batch calls "
                     "between one event pair (enqueue-bound at these sizes: a floor for the kernel's rate) and the algorithmic bytes over "
                     "it, copy_* a device-to-device copy moving as many bytes in the same run (frames stay in the Infinity Cache)",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "batch": args.batch, "warmup": args.warmup,
           "slower_rows": [{k: r[k] for k in ("row", "H", "W", "R") if k in r} for r in losers], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
