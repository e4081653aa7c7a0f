#!/usr/bin/env python3
"""A picture into the texture, three ways, timed in the same process (retexture.py:48-58 with change_texture):

  cross rows    r = 300 -> R = 1024 (the size of the reference's mosaic.png, the C3 / C2 texture) and r = 600 -> R = 2048 (pure.png,
                C5), modes 0 and 3:
      (a) host      the reference's lines as this repository ships them: texture_io.resize_bilinear_u8 of the whole cross on the host,
                    upload of the float cross, texture_io.change_texture on the device.  It takes seconds, so --host-reps (5)
                    repetitions; the resize does not depend on the mode and is timed once per repetition and size, then counted
                    in both modes' rows.
      (b) torch     a torch-only composition on the device, for timing only (it does not quantise, so its values differ): upload of
                    the bytes, F.interpolate(bilinear), change_texture.
      (c) ours      upload of the bytes, texgs.retexture.retexture_cross_u8: one launch.
  lat-long row  512 x 1024 -> R = 1024, mode -1, the picture already on the device:
      (b) torch     latlong_to_cubemap's lines in float32 torch with F.grid_sample (border padding: no wrap, timing only).
      (c) ours      texgs.retexture.retexture_latlong: one launch.

Host wall clock around work that ends synchronised; (b) and (c) alternate inside one loop, --reps (30) repetitions; medians with
p10-p90.  A row counts as faster (or slower) only when the medians differ by more than the OTHER leg's own p10-p90 spread; inside it
the row is a tie.  Also one device-to-device copy of the texture's bytes, as a yardstick for the launch.

--trace: only leg (c), --trace-calls calls per row, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_retexture.py --trace`.
--reduce-trace CSV --out FILE [--label BUILD] [--append]: the per-dispatch kernel_trace.csv of such a run -> one line per row (profiles/retexture_kernel_stats.csv)
with the median kernel time, the byte floor (6 R^2 24 B of texture, 12 B with mode -1, plus the source bytes) and, with --copy-gbs (the
bandwidth scripts/ubench/stream_bw.hip measured in the same session), the fraction of it reached.

Writes profiles/retexture_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_retexture.py [--reps 30] [--host-reps 5] [--warmup 3] [--out FILE] [--trace] [--reduce-trace CSV]"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
CROSS_SIZES = [(300, 1024), (600, 2048)]
CROSS_MODES = [0, 3]
LATLONG = (512, 1024, 1024)         # h, w, R


def floor_bytes(R, mode, src_bytes):
    return 6 * R * R * (12 if mode == -1 else 24) + src_bytes


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_p90_ms": [round(float(np.percentile(v, q)), 4) for q in (10, 90)], "reps": len(v)}


def verdict(ours, other):
    """ours against `other`, by the other leg's own spread"""
    spread = other["p10_p90_ms"][1] - other["p10_p90_ms"][0]
    d = other["median_ms"] - ours["median_ms"]
    return "tie" if abs(d) <= spread else ("faster" if d > 0 else "slower")


def trace_rows():
    return [("cross", r, R, m, 36 * r * r) for r, R in CROSS_SIZES for m in CROSS_MODES] + [("latlong", LATLONG[0], LATLONG[2], -1, LATLONG[0] * LATLONG[1] * 12)]


def reduce_trace(path, out, copy_gbs, calls, label, append):
    """rocprofv3's per-dispatch kernel_trace.csv of a --trace run -> one line per row of trace_rows(): the stats table sums a kernel
    over every size, so the dispatches are taken in launch order, `calls` per row"""
    with open(path) as f:
        recs = list(csv.DictReader(f))
    col = lambda want: next(k for k in recs[0] if k.lower().replace("_", "") == want)      # noqa: E731
    name, start, end = col("kernelname"), col("starttimestamp"), col("endtimestamp")
    ours = sorted((r for r in recs if "k_retexture" in r[name]), key=lambda r: int(r[start]))
    want = trace_rows()
    if len(ours) != calls * len(want):
        raise SystemExit(f"{len(ours)} dispatches of the retexture kernels in {path}, expected {calls} x {len(want)}")
    with open(out, "a" if append else "w", newline="") as f:
        w = csv.writer(f)
        if not append:
            w.writerow(["build", "row", "src", "R", "mode", "kernel", "calls", "median_us", "min_us", "max_us", "floor_bytes", "floor_gbs_at_median",
                        "copy_gbs", "fraction_of_copy_bandwidth"])
        for i, (kind, src, R, mode, src_bytes) in enumerate(want):
            grp = ours[i * calls:(i + 1) * calls]
            us = np.array([(int(r[end]) - int(r[start])) / 1e3 for r in grp])
            fb = floor_bytes(R, mode, src_bytes)
            gbs = fb / (float(np.median(us)) * 1e3)
            kernel = "k_retexture_cross" if "k_retexture_cross" in grp[0][name] else "k_retexture_latlong"
            w.writerow([label, kind, src, R, mode, kernel, calls, round(float(np.median(us)), 2), round(float(us.min()), 2),
                        round(float(us.max()), 2), fb, round(gbs, 1), copy_gbs, "" if not copy_gbs else round(gbs / copy_gbs, 3)])
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions of legs (b) and (c)")
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of leg (a)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retexture_bench.json"))
    ap.add_argument("--trace", action="store_true", help="run only leg (c) (for a profiler)")
    ap.add_argument("--trace-calls", type=int, default=20)
    ap.add_argument("--reduce-trace", metavar="CSV")
    ap.add_argument("--copy-gbs", type=float, default=None)
    ap.add_argument("--label", default="product", help="--reduce-trace: the `build` column (an experiment build's flag)")
    ap.add_argument("--append", action="store_true", help="--reduce-trace: add the rows to an existing file")
    args = ap.parse_args()
    if args.reduce_trace:
        return reduce_trace(args.reduce_trace, args.out, args.copy_gbs, args.trace_calls, args.label, args.append)

    import torch
    from texgs import retexture, texture_io
    if not torch.cuda.is_available():
        raise SystemExit("bench_retexture.py needs an MI355X: there is no CPU path to time")
    F = torch.nn.functional

    def wall_ms(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    rng = np.random.default_rng(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    h, w, RL = LATLONG
    pic = torch.rand(h, w, 3, device=DEV)

    if args.trace:              # the rows of trace_rows(), in that order: --reduce-trace takes the dispatches in launch order
        for r, R in CROSS_SIZES:
            cross = torch.from_numpy(rng.integers(0, 256, (3 * r, 4 * r, 3), dtype=np.uint8)).to(DEV)
            tex = torch.randn(6, R, R, 3, device=DEV)
            for mode in CROSS_MODES:
                for _ in range(args.trace_calls):
                    retexture.retexture_cross_u8(tex, cross, mode=mode, out=tex)
        out = torch.empty(6, RL, RL, 3, device=DEV)
        for _ in range(args.trace_calls):
            retexture.retexture_latlong(pic, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "done", "rows": [list(t[:4]) for t in trace_rows()], "calls_each": args.trace_calls}))
        return

    for r, R in CROSS_SIZES:
        cross_np = rng.integers(0, 256, (3 * r, 4 * r, 3), dtype=np.uint8)
        tex = torch.randn(6, R, R, 3, device=DEV)
        out = torch.empty_like(tex)
        # a device copy of the texture's bytes: what one read and one write of it cost
        copy = [wall_ms(lambda: out.copy_(tex)) for _ in range(args.reps + args.warmup)][args.warmup:]
        # leg (a), the mode-independent part
        resized, t_resize = None, []
        for _ in range(args.host_reps):
            t = time.perf_counter()
            resized = texture_io.resize_bilinear_u8(cross_np, 3 * R, 4 * R)
            t_resize.append((time.perf_counter() - t) * 1e3)
        for mode in CROSS_MODES:
            def host_rest():
                c = torch.tensor(resized.astype(np.float32) / 255.0, device=DEV)
                return texture_io.change_texture(tex, c, mode)

            def torch_leg():
                b = torch.from_numpy(cross_np).to(DEV)
                c = F.interpolate(b.permute(2, 0, 1)[None].float(), size=(3 * R, 4 * R), mode="bilinear", align_corners=False)[0].permute(1, 2, 0) / 255.0
                return texture_io.change_texture(tex, c, mode)

            def ours():
                return retexture.retexture_cross_u8(tex, torch.from_numpy(cross_np).to(DEV), mode=mode, out=out)

            for _ in range(args.warmup):
                host_rest(), torch_leg(), ours()
            t_rest = [wall_ms(host_rest) for _ in range(args.host_reps)]
            t_b, t_c = [], []
            for _ in range(args.reps):
                t_b.append(wall_ms(torch_leg))
                t_c.append(wall_ms(ours))
            a = stats([x + y for x, y in zip(t_resize, t_rest)])
            b, c = stats(t_b), stats(t_c)
            cross_dev = torch.from_numpy(cross_np).to(DEV)
            launch = [wall_ms(lambda: retexture.retexture_cross_u8(tex, cross_dev, mode=mode, out=out)) for _ in range(args.reps)]
            emit({"row": "cross", "r": r, "R": R, "mode": mode, "host": a, "host_resize_only": stats(t_resize), "torch": b, "ours": c,
                  "ours_launch_only": stats(launch), "device_copy_of_the_texture": stats(copy),
                  "floor_bytes": floor_bytes(R, mode, cross_np.size),
                  "host_over_ours": round(a["median_ms"] / c["median_ms"], 1), "torch_over_ours": round(b["median_ms"] / c["median_ms"], 3),
                  "verdict_against_host": verdict(c, a), "verdict_against_torch": verdict(c, b)})
        del tex, out
        torch.cuda.empty_cache()

    # ---- the lat-long picture ----
    out = torch.empty(6, RL, RL, 3, device=DEV)

    def cube_to_dir(s, x, y):
        one = torch.ones_like(x)
        return torch.stack([(one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one)][s], dim=-1)

    def torch_latlong():
        cube = torch.zeros(6, RL, RL, 3, device=DEV)
        lin = torch.linspace(-1.0 + 1.0 / RL, 1.0 - 1.0 / RL, RL, device=DEV)
        for s in range(6):
            gy, gx = torch.meshgrid(lin, lin, indexing="ij")
            v = F.normalize(cube_to_dir(s, gx, gy), dim=-1)
            tu = torch.atan2(v[..., 0:1], -v[..., 2:3]) / (2 * math.pi) + 0.5
            tv = torch.acos(torch.clamp(v[..., 1:2], min=-1, max=1)) / math.pi
            grid = torch.cat((tu, tv), dim=-1)[None] * 2 - 1
            cube[s] = F.grid_sample(pic.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0)
        return texture_io.rgb2sh0(cube)

    def ours_latlong():
        return retexture.retexture_latlong(pic, out=out)

    for _ in range(args.warmup):
        torch_latlong(), ours_latlong()
    t_b, t_c = [], []
    for _ in range(args.reps):
        t_b.append(wall_ms(torch_latlong))
        t_c.append(wall_ms(ours_latlong))
    b, c = stats(t_b), stats(t_c)
    emit({"row": "latlong", "h": h, "w": w, "R": RL, "mode": -1, "torch": b, "ours": c, "floor_bytes": floor_bytes(RL, -1, pic.numel() * 4),
          "torch_over_ours": round(b["median_ms"] / c["median_ms"], 3), "verdict_against_torch": verdict(c, b),
          # faces 0, 1 and 5 have no texel at the seam, where the torch leg's border padding cannot wrap
          "largest_difference_between_legs_on_faces_0_1_5": float((torch_latlong() - ours_latlong())[[0, 1, 5]].abs().max())})

    res = {"metric": "host wall-clock ms of work that ends synchronised; medians and p10-p90; legs (b) and (c) alternate in one process; "
                     "a verdict is against the other leg's own p10-p90 spread",
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "reps": args.reps, "host_reps": args.host_reps,
           "warmup": args.warmup,
           "not_faster_rows": [{k: r.get(k) for k in ("row", "R", "mode")} for r in rows
                               if "faster" != r.get("verdict_against_torch") or r.get("verdict_against_host", "faster") != "faster"],
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
