#!/usr/bin/env python3
"""The colour stage two ways, timed in the same process on the same tensors: texgs.shcolor against the torch composition of the
render glue's `convert_SHs_python` branch under autograd (tests/shcolor_ref.torch_lines: the chain of elementwise launches the
reference executes, about sixty at degree 3).

  rows      N = 300 000 and 1 000 000;  degree 3 / K = 16 and degree 4 / K = 25;  one view per call (sh_colors) and 8 views
            (sh_colors_views against 8 torch chains);  forward alone (under no_grad) and forward + backward (gradients to the
            features and to xyz, the same upstream gradients into both legs).
  timing    host wall clock around work that ends synchronised, the two legs alternating inside one loop; medians with p10-p90 of
            --reps repetitions.  verdict: "faster" / "slower" when the medians differ by more than the TORCH leg's own p10-p90
            spread, "tie" inside it.
  floor     the bytes the stage must move (coefficient rows, xyz, colours; for the backward also the upstream gradients and the
            two gradient outputs) over the stream bandwidth measured in this run (a device-to-device copy of 1 GiB, read + written
            bytes over its median time); `fraction_of_byte_floor` = that time / the stage's median.
The legs' results are compared in this run (largest absolute difference of the colours, relative L2 of the gradients); the bit-exact
comparison is the test suite's.

Writes profiles/shcolor_bench.json (or --out) and prints one JSON line per row.
Usage: python scripts/bench_shcolor.py [--reps 30] [--warmup 3] [--sizes 300000,1000000] [--degrees 3,4] [--forward-only] [--out FILE]
(TEXGS_LIB=path selects an experiment build of the library, as everywhere.)"""
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

import shcolor_ref as R  # noqa: E402
from texgs import shcolor  # noqa: E402

DEV = "cuda:0"


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_p90_ms": [round(float(np.percentile(v, q)), 4) for q in (10, 90)]}


def verdict(r, o):
    """Against the torch leg's own spread"""
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
    return {"torch": r, "shcolor": o, "torch_minus_shcolor_ms": round(r["median_ms"] - o["median_ms"], 4),
            "torch_over_shcolor": round(r["median_ms"] / o["median_ms"], 3), "verdict": verdict(r, o)}


def stream_bandwidth():
    """Bytes per second of a device-to-device copy of 1 GiB (read + written bytes over the median wall time of 20 copies)"""
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    t = [wall_ms(lambda: dst.copy_(src)) for _ in range(20)]
    return 2.0 * src.numel() * 4 / (float(np.median(t)) * 1e-3)


def norm_diff(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions per row")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="300000,1000000")
    ap.add_argument("--degrees", default="3,4", help="degrees to time (K = (degree + 1)^2)")
    ap.add_argument("--forward-only", action="store_true", help="skip the forward + backward rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shcolor_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shcolor.py needs an MI355X: there is no CPU path to time")
    bw = stream_bandwidth()
    print(json.dumps({"stream_bandwidth_TBps": round(bw / 1e12, 3)}), flush=True)
    rows = []
    for N in [int(s) for s in args.sizes.split(",")]:
        for deg, K in [(int(d), (int(d) + 1) ** 2) for d in args.degrees.split(",")]:
            g = torch.Generator().manual_seed(N + K)
            feats = torch.randn(N, K, 3, generator=g).to(DEV).requires_grad_(True)
            u = torch.randn(N, 3, generator=g)
            xyz = (u / u.norm(dim=1, keepdim=True) * (2.0 + 4.0 * torch.rand(N, 1, generator=g))).to(DEV).requires_grad_(True)
            for V in (1, 8):
                cams = (torch.rand(V, 3, generator=g) * 2 - 1).to(DEV)
                ups = torch.randn(V, N, 3, generator=g).to(DEV)

                def torch_fwd():
                    with torch.no_grad():
                        return torch.stack([R.torch_lines(feats, xyz, cams[v], deg) for v in range(V)])

                def hip_fwd():
                    with torch.no_grad():
                        return shcolor.sh_colors_views(feats, xyz, cams, deg) if V > 1 else shcolor.sh_colors(feats, xyz, cams[0], deg)[None]

                def grads(cols, keep):
                    torch.autograd.backward([cols], [ups])
                    out = (feats.grad, xyz.grad)
                    feats.grad = xyz.grad = None
                    return out if keep else None

                def torch_both(keep=False):
                    return grads(torch.stack([R.torch_lines(feats, xyz, cams[v], deg) for v in range(V)]), keep)

                def hip_both(keep=False):
                    return grads(shcolor.sh_colors_views(feats, xyz, cams, deg) if V > 1 else shcolor.sh_colors(feats, xyz, cams[0], deg)[None], keep)

                a, b = torch_fwd(), hip_fwd()
                ga, gb = torch_both(keep=True), hip_both(keep=True)
                diff = {"colours_max_abs": float((a - b).abs().max()), "d_features_rel_l2": norm_diff(gb[0], ga[0]),
                        "d_xyz_rel_l2": norm_diff(gb[1], ga[1])}
                fwd_bytes = N * (12 * K + 12 + 12 * V)
                bwd_bytes = N * (12 * K + 12 + 12 * V + 12 * K + 12)
                legs = [("forward", torch_fwd, hip_fwd, fwd_bytes), ("forward+backward", torch_both, hip_both, fwd_bytes + bwd_bytes)]
                for what, ref, ours, nbytes in legs[:1] if args.forward_only else legs:
                    row = {"row": what, "N": N, "degree": deg, "K": K, "views": V, "shcolor_launches": 1 if what == "forward" else 2,
                           "difference_between_legs": diff, "bytes": nbytes}
                    row.update(alternate(ref, ours, args.reps, args.warmup))
                    floor_ms = nbytes / bw * 1e3
                    row["byte_floor_ms"] = round(floor_ms, 4)
                    row["fraction_of_byte_floor"] = round(floor_ms / row["shcolor"]["median_ms"], 3)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del cams, ups, a, b, ga, gb
            del feats, xyz
            torch.cuda.empty_cache()
    out = {"metric": "host wall-clock ms of work that ends synchronised; medians and p10-p90 of alternating repetitions in one process; "
                     "verdict against the torch leg's own p10-p90 spread; byte floor at the stream bandwidth measured in this run",
           "device": torch.cuda.get_device_name(0), "library": os.environ.get("TEXGS_LIB") or "in-tree", "host_threads": torch.get_num_threads(), "reps": args.reps, "warmup": args.warmup,
           "stream_bandwidth_TBps": round(bw / 1e12, 3), "stream_bandwidth_method": "device-to-device copy of 1 GiB, read + written bytes",
           "slower_rows": [{k: r[k] for k in ("row", "N", "degree", "views")} for r in rows if r["verdict"] == "slower"],
           "tied_rows": [{k: r[k] for k in ("row", "N", "degree", "views")} for r in rows if r["verdict"] == "tie"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
