#!/usr/bin/env python3
"""The point-cloud operations between the stages (texgs.points: 3-NN scale initialisation, farthest-point sampling) against the
plain-torch form of the same statements, timed in the same process:

  hip       texgs.points.knn3_mean_dist2 / sample_farthest_points (csrc/points.hip)
  baseline  3-NN: chunked ((a[:, None] - b[None]) ** 2).sum(-1) + topk(4, largest=False), the self distance dropped;
            FPS:  the torch loop of the statement (minimum, argmax)

Rows: 3-NN at N in {100 k, 300 k, 1 M} x {uniform, clustered}; FPS at K = 16 384 for N = 300 k clustered and N = 1 M clustered.
Clouds are seeded and generated here.  Every shape is warmed up on both paths before it is timed; the timed calls alternate
hip / baseline; every timing is wall clock around one call and a device synchronise (the FPS loop is host-bound: wall clock is
what a user waits for).  Rows whose results differ (3-NN: not within 1e-5 relative; FPS: other points picked) are marked.

Writes profiles/points_bench.json (or --out) and prints one JSON summary line.
--trace: run only the HIP path once per shape, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_points.py --trace`.
Usage: python scripts/bench_points.py [--reps 5] [--quick] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import points  # noqa: E402


def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def clustered(n, seed):
    """12 Gaussian clusters, per-point spreads from {1e-3, 0.02, 0.3}, 1 % outliers at sigma = 60, 2 % exact duplicates"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-4.0, 4.0, (12, 3))
    p = centres[rng.integers(0, 12, n)] + rng.standard_normal((n, 3)) * rng.choice(np.array([1e-3, 0.02, 0.3]), n)[:, None]
    out = rng.choice(n, max(1, n // 100), replace=False)
    p[out] = rng.standard_normal((out.size, 3)) * 60.0
    p = p.astype(np.float32)
    dst = rng.choice(n, max(1, n // 50), replace=False)
    p[dst] = p[rng.integers(0, n, dst.size)]
    return np.ascontiguousarray(p)


def torch_knn3(x):
    n = x.shape[0]
    chunk = max(1, (1 << 27) // n)                 # [chunk, N, 3] fp32 of about 1.5 GB
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    for lo in range(0, n, chunk):
        d = ((x[lo:lo + chunk, None] - x[None]) ** 2).sum(-1)
        out[lo:lo + chunk] = d.topk(4, dim=1, largest=False).values[:, 1:].mean(1)      # [:, 0] is the point itself
    return out


def torch_fps(x, k, start=0):
    n = x.shape[0]
    idx = torch.empty(k, dtype=torch.int64, device=x.device)
    idx[0] = start
    m = torch.full((n,), float("inf"), dtype=torch.float32, device=x.device)
    for t in range(1, k):
        m = torch.minimum(m, ((x - x[idx[t - 1]]) ** 2).sum(-1))
        idx[t] = torch.argmax(m)
    return idx


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls of the HIP path per row (the baseline: 3, one at N = 1 M)")
    ap.add_argument("--quick", action="store_true", help="leave the N = 1 M rows out")
    ap.add_argument("--trace", action="store_true", help="the HIP path once per shape, nothing written (for a profiler)")
    ap.add_argument("--only", choices=["knn3", "fps"], help="rows of one operation only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gens = {"uniform": uniform, "clustered": clustered}
    sizes = [100_000, 300_000] + ([] if args.quick else [1_000_000])
    work = [("knn3", n, c, None) for n in sizes for c in ("uniform", "clustered")]
    work += [("fps", n, "clustered", 16384) for n in sizes[1:]]
    if args.only:
        work = [w for w in work if w[0] == args.only]

    if args.trace:
        for op, n, cloud, k in work:
            x = torch.from_numpy(gens[cloud](n, 1)).to(dev)
            r = points.knn3_mean_dist2(x) if op == "knn3" else points.sample_farthest_points(x, k)[1]
            torch.cuda.synchronize()
            print(op, n, cloud, k, tuple(r.shape), flush=True)
        return

    rows = []
    for op, n, cloud, k in work:
        x = torch.from_numpy(gens[cloud](n, 1)).to(dev)
        if op == "knn3":
            hip, base = (lambda: points.knn3_mean_dist2(x)), (lambda: torch_knn3(x))
        else:
            hip, base = (lambda: points.sample_farthest_points(x, k)[1]), (lambda: torch_fps(x, k))
        _, r_hip = timed(hip)                       # warm-up of this shape, both paths
        _, r_base = timed(base)
        if op == "knn3":
            agree = bool(torch.allclose(r_hip, r_base, rtol=1e-5, atol=0))
        else:       # the same POINTS (among exact duplicates torch.argmax need not return the lowest index)
            agree = bool(torch.equal(x[r_hip], x[r_base]))
        n_base = 1 if n >= 1_000_000 else 3
        t_hip, t_base = [], []
        for i in range(max(args.reps, n_base)):     # alternating
            if i < args.reps:
                t_hip.append(timed(hip)[0])
            if i < n_base:
                t_base.append(timed(base)[0])
        row = {"op": op, "N": n, "cloud": cloud, "hip_ms": round(float(np.median(t_hip)), 4), "baseline_ms": round(float(np.median(t_base)), 4),
               "hip_all_ms": [round(t, 4) for t in t_hip], "baseline_all_ms": [round(t, 4) for t in t_base], "results_agree": agree}
        if k:
            row["indices_equal"] = bool(torch.equal(r_hip, r_base))
            row["K"] = k
            row["hip_us_per_pick"] = round(row["hip_ms"] * 1e3 / (k - 1), 3)
            row["baseline_us_per_pick"] = round(row["baseline_ms"] * 1e3 / (k - 1), 3)
        row["speedup_vs_baseline"] = round(row["baseline_ms"] / row["hip_ms"], 2)
        row["hip_faster"] = row["hip_ms"] < row["baseline_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, r_hip, r_base
        torch.cuda.empty_cache()
    out = {"metric": "texgs.points against plain torch, wall-clock ms per call (median)", "device": torch.cuda.get_device_name(0),
           "reps_hip": args.reps, "rows": rows, "hip_faster_on_every_row": all(r["hip_faster"] for r in rows),
           "results_agree_on_every_row": all(r["results_agree"] for r in rows)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
