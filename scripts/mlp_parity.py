#!/usr/bin/env python3
"""The fused MLP's measured error per shape, in the unit tests/test_mlp_gpu.py bounds it in:

    ratio = max|hip - f64| / max( max|cpu_f32 - f64|, 2^-23 max|f64| )          (the tests' bound is ratio <= 4)

for y, dx and d_params, over the shapes and the tile-edge sizes of the tests plus the size at which a workgroup of the backward's
persistent grid runs a second tile.  f64 and cpu_f32 are tests/mlp_ref.py's two modes on the same kink-free inputs.

Writes profiles/mlp_parity.json (or --out) and prints one JSON summary line.  Usage: python scripts/mlp_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mlp_ref as R  # noqa: E402
from texgs import mlp  # noqa: E402

SPECS = [(3, 128, 1), (32, 128, 1), (128, 3, 2), (128, 128, 2), (16, 16, 1), (1, 1, 2), (17, 33, 2)]


def ratios(spec, N, seed):
    params, x = R.kink_free_inputs(spec, N, seed)
    dy = np.random.default_rng(seed + 1).standard_normal((N, spec[1])).astype(np.float32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    pt = torch.from_numpy(params).cuda().requires_grad_(True)
    y = mlp.fused_mlp(xt, pt, *spec)
    y.backward(torch.from_numpy(dy).cuda())
    f64 = (R.forward(params, x, spec),) + R.backward(params, x, dy, spec)
    f32 = (R.forward(params, x, spec, fp32=True),) + R.backward(params, x, dy, spec, fp32=True)
    out = {}
    for name, got, a, b in zip(("y", "dx", "d_params"), (y, xt.grad, pt.grad), f64, f32):
        err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - a).max())
        out[name] = {"max_abs_err": err, "ratio": round(4 * err / R.tolerance(a, b), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_parity.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_parity.py needs an MI355X")
    T, B, G = mlp.FORWARD_TILE, mlp.BACKWARD_TILE, mlp.BACKWARD_MAX_WORKGROUPS
    sizes = sorted({1, B - 1, B, B + 1, 2 * B + 1, T - 1, T, T + 1, 2 * T + 1})
    rows, worst = {}, 0.0
    for spec in SPECS:
        per = {}
        for N in sizes + ([B * G + B + 1] if spec == (128, 128, 2) else []):
            per[str(N)] = r = ratios(spec, N, seed=100 + N)
            worst = max(worst, *(v["ratio"] for v in r.values()))
        rows["x".join(map(str, spec))] = {"worst_ratio": max(v["ratio"] for r in per.values() for v in r.values()), "by_N": per}
    out = {"metric": "max|hip - f64| over max(max|cpu_f32 - f64|, 2^-23 max|f64|); tests/test_mlp_gpu.py requires <= 4",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "bound": 4, "worst_ratio": worst,
           "shapes (n_in x n_out x hidden layers)": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"parity": "mlp", "worst_ratio": worst, **{k: v["worst_ratio"] for k, v in rows.items()}}))


if __name__ == "__main__":
    main()
