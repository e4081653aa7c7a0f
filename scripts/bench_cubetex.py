#!/usr/bin/env python3
"""sphere_map (texgs.cubetex; models/texture_gaussian3d.py:446-449) two ways, timed in the same process:

  fused     texgs.cubetex.sphere_map(texture): one launch, sh02rgb on every tap, the directions computed in the kernel
  composed  cube_sample(sh02rgb(texture), latlong_dirs(resolution)): what the reference does with nvdiffrast -- the whole texture
            converted first (6 R R 3 floats read and written: 75 MB each at R = 1024), the direction tensor built, then the fetch

Rows: R = 1024 and R = 2048, output (512, 1024), a seeded random sh0 texture in [-3, 3] (both clamps of sh02rgb fire).  Both paths
are warmed up at every shape; the timed windows alternate fused / composed.  Two figures per path:

  *_ms          one call between a pair of device events, after a synchronise: the per-call LATENCY on an idle queue.  The composed
                path is about fifteen launches (three elementwise kernels, the small kernels of latlong_dirs, the fetch), so its
                figure includes the host's launch gaps, not only device work.
  *_batched_ms  --batch calls enqueued between one pair of events, divided by their number: the queue stays full, so this is
                device work per call.

What the figures do not say: calls run back to back here, so a 75 MB texture (R = 1024) stays in the 256 MB Infinity Cache between
them, whereas retexture.py renders a view between two calls; and latlong_dirs builds its grid in float64 on every call where the
reference builds it in fp32 (a few small kernels on 512 x 1024 elements either way).  Both favour neither path by much at
R = 1024 but blur the ratio; read it as an order of magnitude.
The expectation that the fused path wins rests on byte counts only; the ratio is written down whichever way it comes out.
Rows whose two results differ by more than the forward bound of the fetch (tests/test_cubetex_gpu.py) are marked.

Writes profiles/cubetex_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_cubetex.py [--iters 1000] [--batch 20] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import cubetex  # noqa: E402

SH_C0 = 0.28209479177387814


def sh02rgb(sh0):
    return torch.clamp(SH_C0 * sh0 + 0.5, 0.0, 1.0)


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def batch_ms(f, k):
    """k calls enqueued between one pair of events: ms per call with the queue kept full"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(k):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000, help="timed calls of each path per row")
    ap.add_argument("--batch", type=int, default=20, help="calls per batched window (iters / batch windows per path)")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of each path per row")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cubetex_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = (512, 1024)
    rows = []
    for R in args.sizes:
        g = torch.Generator().manual_seed(R)
        tex = (torch.rand(6, R, R, 3, generator=g) * 6.0 - 3.0).to(dev)
        fused = lambda: cubetex.sphere_map(tex, res)                                                   # noqa: E731
        composed = lambda: cubetex.cube_sample(sh02rgb(tex), cubetex.latlong_dirs(res, dev))          # noqa: E731
        for _ in range(args.warmup):
            fused(), composed()
        diff = float((fused() - composed()).abs().max())          # (synchronises)
        bound = 8.0 * 2.0 ** -23 * (R / 2.0) + 8.0 * 2.0 ** -23         # the forward bound for values in [0, 1]
        t_f, t_c = [], []
        for _ in range(args.iters):                 # alternating
            t_f.append(event_ms(fused)[0])
            t_c.append(event_ms(composed)[0])
        b_f, b_c = [], []
        for _ in range(max(1, args.iters // args.batch)):
            b_f.append(batch_ms(fused, args.batch))
            b_c.append(batch_ms(composed, args.batch))
        row = {"R": R, "resolution": list(res), "fused_ms": round(float(np.median(t_f)), 4), "composed_ms": round(float(np.median(t_c)), 4),
               "fused_p10_p90_ms": [round(float(np.percentile(t_f, q)), 4) for q in (10, 90)],
               "composed_p10_p90_ms": [round(float(np.percentile(t_c, q)), 4) for q in (10, 90)],
               "texture_mb": round(tex.numel() * 4 / 1e6, 1), "max_abs_difference": diff, "results_agree": diff <= bound}
        row["fused_batched_ms"] = round(float(np.median(b_f)), 4)
        row["composed_batched_ms"] = round(float(np.median(b_c)), 4)
        row["composed_over_fused"] = round(row["composed_ms"] / row["fused_ms"], 2)
        row["composed_over_fused_batched"] = round(row["composed_batched_ms"] / row["fused_batched_ms"], 2)
        row["fused_faster"] = row["fused_ms"] < row["composed_ms"] and row["fused_batched_ms"] < row["composed_batched_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del tex
        torch.cuda.empty_cache()
    out = {"metric": "sphere_map fused against cube_sample(sh02rgb(texture), latlong_dirs), device-event ms per call (median): *_ms = latency of one "
                     "call on an idle queue, launch gaps included; *_batched_ms = per call with --batch calls enqueued between one event pair; "
                     "calls run back to back (the texture may stay in the Infinity Cache)", "batch": args.batch,
           "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "rows": rows,
           "fused_faster_on_every_row": all(r["fused_faster"] for r in rows),
           "results_agree_on_every_row": all(r["results_agree"] for r in rows)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
