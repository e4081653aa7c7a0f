#!/usr/bin/env python3
"""The surface-point stage two ways, timed in the same process: the reference's own lines (texgs.losses.depth2world -- arange,
meshgrid, stack, a 4x4 linalg.inv, an [HW,4] x [4,4] product -- and the two boolean indexings of uv_map_gaussian3d.py:274-277) against
texgs.surface.surface_points (three HIP launches, one host wait).

  points     depth and alpha of a texgs.synth scene's untextured render at 800x800 and 1600x1200 -> world points and pixel indices of
             the pixels with alpha > 0.5.  Host wall clock around a call that ends synchronised (the reference leg's cost is largely
             its host waits), the two legs alternating inside one loop; medians with p10-p90.
             verdict: "faster" / "slower" when the medians differ by more than the REFERENCE leg's own p10-p90 spread, "tie" inside it.
  device     device-event time per call, --batch calls between one event pair: surface_points(wait=False) (no host wait inside the
             batch) and the reference's lines (their host waits included: they cannot be taken out), and the algorithmic bytes of
             the three launches over the former
  compose    uv_map_gaussian3d.py:283-286 (repeat, scatter_add, permute) against texgs.surface.compose, same protocol as `points`

The results of the two legs are compared in this run (largest difference, and both against a float64 torch computation); the
bit-exact comparison is the test suite's.

Writes profiles/surface_bench.json (or --out) and prints one JSON summary line.
--trace: only the HIP path, 50 calls at 1600x1200, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_surface.py --trace`
(profiles/surface_kernel_stats.csv is that run's kernel table).
Usage: python scripts/bench_surface.py [--reps 30] [--batch 20] [--warmup 3] [--out FILE] [--trace]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import losses, surface, synth, uvmap  # noqa: E402
from texgs.rasterizer import GaussianRasterizationSettings  # noqa: E402

DEV = "cuda:0"


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


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_p90_ms": [round(float(np.percentile(v, q)), 4) for q in (10, 90)]}


def verdict(r, o):
    """Against the reference leg's own spread"""
    spread = r["p10_p90_ms"][1] - r["p10_p90_ms"][0]
    d = r["median_ms"] - o["median_ms"]
    return "tie" if abs(d) <= spread else ("faster" if d > 0 else "slower")


def alternate(ref, ours, reps, warmup):
    for _ in range(warmup):
        ref(), ours()
    t_ref, t_ours = [], []
    for _ in range(reps):
        t_ref.append(wall_ms(ref))
        t_ours.append(wall_ms(ours))
    r, o = stats(t_ref), stats(t_ours)
    return {"reference": r, "surface": o, "reference_over_surface": round(r["median_ms"] / o["median_ms"], 2), "verdict": verdict(r, o)}


def render(W, H):
    """The untextured render of a synthetic scene: (depth [1,H,W], alpha [1,H,W], full_proj [4,4]) on the device"""
    scene = synth.make_scene(20000, 4, seed=7, scale_mean=0.03)
    cam = synth.fibonacci_cameras(6, W, H)[2]
    f = lambda t: t.float().to(DEV).contiguous()        # noqa: E731
    st = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
                                       tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.zeros(3, device=DEV), scale_modifier=1.0,
                                       viewmatrix=f(cam.world_view_transform), projmatrix=f(cam.full_proj_transform), sh_degree=0,
                                       campos=f(cam.camera_center), prefiltered=False, debug=False)
    depth, alpha = uvmap.render_depth_alpha(st, f(scene.means3D), f(scene.opacities), f(scene.scales), f(scene.rotations))
    return depth.contiguous(), alpha.contiguous(), f(cam.full_proj_transform)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions per row")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.json"))
    ap.add_argument("--trace", action="store_true", help="run only the HIP path (for a profiler)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py needs an MI355X: there is no CPU path to time")
    zfar, znear = 100.0, 0.01
    if args.trace:
        depth, alpha, proj = render(1600, 1200)
        for _ in range(50):
            pts = surface.surface_points(depth, alpha, proj, zfar, znear, with_rank=True)
            surface.compose(pts, pts.xyz, alpha, [0.25, 0.5, 0.125])
        torch.cuda.synchronize()
        print(json.dumps({"trace": "done", "image": [1200, 1600], "selected": pts.count, "calls": 50}))
        return
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for W, H in ((800, 800), (1600, 1200)):
        depth, alpha, proj = render(W, H)
        n = H * W
        shape = {"image": [H, W]}

        def ref():              # uv_map_gaussian3d.py:271-277
            world = losses.depth2world(depth.squeeze(0), proj, zfar, znear)
            valid = alpha.reshape(-1) > 0.5
            index = torch.arange(n, device=DEV)[valid]
            return world.reshape(-1, 3)[valid], index

        ours = lambda: surface.surface_points(depth, alpha, proj, zfar, znear)          # noqa: E731
        (r_xyz, r_index), pts = ref(), ours()
        M = pts.count
        exact = losses.depth2world(depth.squeeze(0).double(), proj.double(), zfar, znear).reshape(-1, 3)[r_index]
        row = {"row": "points", **shape, "selected": M, "selected_fraction": round(M / n, 4),
               "same_pixels": bool(torch.equal(r_index, pts.index)),
               "max_difference_between_legs": float((r_xyz - pts.xyz).abs().max()),
               "max_error_vs_float64": {"reference": float((r_xyz.double() - exact).abs().max()),
                                        "surface": float((pts.xyz.double() - exact).abs().max())}}
        row.update(alternate(ref, ours, args.reps, args.warmup))
        emit(row)

        held = []
        queued = lambda: held.append(surface.surface_points(depth, alpha, proj, zfar, znear, wait=False))        # noqa: E731
        t_ours = []
        for _ in range(5):
            t_ours.append(batch_ms(queued, args.batch))
            assert all(q.wait() == M for q in held)         # the counts are read only behind the timed batch
            held.clear()
        t_ref = [batch_ms(ref, args.batch) for _ in range(5)]
        quads = int((alpha.reshape(-1) > 0.5).reshape(-1, 4).any(dim=1).sum()) if n % 4 == 0 else (M + 3) // 4
        nbytes = 2 * n * 4 + quads * 16 + M * (12 + 8) + 4 * ((n + 1023) // 1024) * 3
        emit({"row": "device", **shape, "batch": args.batch, "launches": 3,
              "surface_call_batched_ms": round(float(np.median(t_ours)), 4), "reference_call_batched_ms": round(float(np.median(t_ref)), 4),
              "algorithmic_mb": round(nbytes / 1e6, 2), "surface_call_gbps": round(nbytes / (float(np.median(t_ours)) * 1e-3) / 1e9, 1)})

        # the composite: per-point colours back onto the grid
        rgb = torch.rand(M, 3, device=DEV)
        bg = torch.tensor([0.25, 0.5, 0.125], device=DEV)
        with_rank = surface.surface_points(depth, alpha, proj, zfar, znear, with_rank=True)

        def ref_compose():      # uv_map_gaussian3d.py:283-286
            src = alpha.reshape(-1)[r_index][:, None] * rgb
            img = bg.reshape(1, 3).repeat(n, 1) * (1 - alpha).reshape(-1, 1)
            img = img.scatter_add(dim=0, index=r_index[:, None].repeat(1, 3), src=src)
            return img.reshape(H, W, 3).permute(2, 0, 1)

        ours_compose = lambda: surface.compose(with_rank, rgb, alpha, bg)       # noqa: E731
        row = {"row": "compose", **shape, "max_difference_between_legs": float((ref_compose() - ours_compose()).abs().max())}
        row.update(alternate(ref_compose, ours_compose, args.reps, args.warmup))
        emit(row)
        del depth, alpha, rgb, with_rank, pts
        torch.cuda.empty_cache()

    out = {"metric": "host wall-clock ms of a call that ends synchronised; medians and p10-p90 of alternating repetitions in one process; "
                     "verdict against the reference leg's own p10-p90 spread; `device` rows: device-event ms per call over a batch",
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "reps": args.reps, "warmup": args.warmup,
           "slower_rows": [{"row": r["row"], "image": r["image"]} for r in rows if r.get("verdict") == "slower"],
           "tied_rows": [{"row": r["row"], "image": r["image"]} for r in rows if r.get("verdict") == "tie"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
