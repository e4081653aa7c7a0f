#!/usr/bin/env python3
"""The fused MLP (texgs.mlp, csrc/mlp.hip) against the torch composition of the same function, on the same GPU in the same process.

Shapes: the four networks the reference builds per model (models/modules/utils.py:18-41) -- 3 -> 128 -> 128, 32 -> 128 -> 128 and
128 -> 128 -> 128 -> 3 (used twice: one row) -- at N = 460 342 points, the stage-2 valid-point count of profiles/uvmap_bench.json.

Cases per shape, on the same fp32 inputs and the same flat parameters:
  fused_fwd / fused_fwd_bwd    texgs.mlp.fused_mlp, forward alone (no graph) / forward + backward to x and params
  torch_fwd / torch_fwd_bwd    the `@` and clamp_min_ chain over the matrices of the flat parameters (ones-padded input, sliced output),
                               under autograd for the backward

Every case is warmed up and the timed repetitions alternate between the cases; a timing is a pair of device events around one call
inside a synchronised window.  Reported: median and minimum over --reps, and the ratio torch / fused of the medians.

Writes profiles/mlp_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_mlp.py [--reps 30] [--warmup 5] [--n 460342] [--out FILE]"""
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

from texgs import mlp  # noqa: E402

SHAPES = [(3, 128, 1), (32, 128, 1), (128, 3, 2)]


def torch_mlp(x, params, n_in, n_out, depth):
    """The same function as a chain of library GEMMs"""
    mats, off = [], 0
    for a, b in mlp.matrix_shapes(n_in, n_out, depth):
        mats.append(params[off:off + a * b].view(a, b))
        off += a * b
    pin = mats[0].shape[1]
    h = torch.cat([x, x.new_ones(x.shape[0], pin - n_in)], dim=1) if pin > n_in else x
    for W in mats[:-1]:
        h = (h @ W.t()).clamp_min_(0)
    return (h @ mats[-1].t())[:, :n_out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=460342)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp.py needs an MI355X: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = {}
    for spec in SHAPES:
        n_in, n_out, depth = spec
        params = mlp.FusedMLP(*spec).params.detach().to(dev).requires_grad_(True)
        x = (torch.rand(a.n, n_in, generator=g, device=dev) * 2 - 1).requires_grad_(True)
        dy = torch.randn(a.n, n_out, generator=g, device=dev)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(x, params, *spec)
            return run

        def fwd_bwd(fn):
            def run():
                x.grad = params.grad = None
                fn(x, params, *spec).backward(dy)
            return run

        cases = {"fused_fwd": fwd(mlp.fused_mlp), "torch_fwd": fwd(torch_mlp), "fused_fwd_bwd": fwd_bwd(mlp.fused_mlp),
                 "torch_fwd_bwd": fwd_bwd(torch_mlp)}

        def timed(run):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            for run in cases.values():
                timed(run)
        ms = {k: [] for k in cases}
        for _ in range(max(a.reps, 1)):
            for k, run in cases.items():            # alternate: drift and other people's work hit every case alike
                ms[k].append(timed(run))
        # the two compute the same thing
        with torch.no_grad():
            ya, yb = mlp.fused_mlp(x, params, *spec), torch_mlp(x, params, *spec)
        agree = float((ya - yb).abs().max() / yb.abs().max())
        row = {k: {"device_ms_median": round(float(np.median(v)), 4), "device_ms_min": round(float(np.min(v)), 4)} for k, v in ms.items()}
        row["torch_over_fused_fwd"] = round(row["torch_fwd"]["device_ms_median"] / row["fused_fwd"]["device_ms_median"], 3)
        row["torch_over_fused_fwd_bwd"] = round(row["torch_fwd_bwd"]["device_ms_median"] / row["fused_fwd_bwd"]["device_ms_median"], 3)
        row["max_rel_diff_fused_vs_torch"] = agree
        rows["%d-%s-%d" % (n_in, "-".join(["128"] * depth), n_out)] = row
    out = {"metric": "one call, device-event ms, median and minimum over the repetitions; torch_over_fused > 1: the fused kernel is faster",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "warmup": a.warmup, "N": a.n, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "mlp", "N": a.n, **{k: {"fwd": r["torch_over_fused_fwd"], "fwd_bwd": r["torch_over_fused_fwd_bwd"],
                                                       "fused_fwd_ms": r["fused_fwd"]["device_ms_median"],
                                                       "fused_fwd_bwd_ms": r["fused_fwd_bwd"]["device_ms_median"]} for k, r in rows.items()}}))


if __name__ == "__main__":
    main()
