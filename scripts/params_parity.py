#!/usr/bin/env python3
"""The parameter stage on the device against the numpy statements of tests/params_ref.py, measured: for every output of the stage,
forward and backward, the error against the float64 statement (max |device - float64| / scale over every element, the scales of
tests/test_params_gpu.py), the float32 statement's own error floored at 2^-24, their ratio (the tests bound it by 4), and whether
the device's bits equal the float32 statement's.

Writes profiles/params_parity.json (or --out) and prints one JSON line per size.
Usage: python scripts/params_parity.py [--sizes 1,2,63,...] [--out FILE]"""
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

import params_ref as R  # noqa: E402
from texgs import params as P  # noqa: E402

DEV = "cuda:0"
EPS, MOD = 1e-3, 0.37


def main():
    rpw = P.ROWS_PER_WORKGROUP
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(n) for n in (1, 2, 63, 64, 65, rpw - 1, rpw, rpw + 1, 3 * rpw + 5, 300000)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("params_parity.py needs an MI355X: there is no CPU path")
    dev = lambda v, grad=False: torch.tensor(np.asarray(v, R.F), device=DEV).requires_grad_(grad)       # noqa: E731
    host = lambda t: t.detach().cpu().numpy()       # noqa: E731
    rows = []
    for N in [int(s) for s in args.sizes.split(",")]:
        a, q, x = R.random_rows(N, 11 + N)
        g = R.random_grads(N, 11 + N)
        fields = R.parity_fields(a, q, x, g, EPS, MOD)
        ta, tq, tx = dev(a, True), dev(q, True), dev(x, True)
        s, r, o, reg = P.activate(ta, tq, tx, opacity_reg=True, epsilon=EPS)
        torch.autograd.backward([s, r, o, reg], [dev(g["g_scales"]), dev(g["g_rotations"]), dev(g["g_opacities"]), dev(g["g_reg"])])
        ca, cq = dev(a, True), dev(q, True)
        cov = P.covariance(ca, cq, MOD)
        cov.backward(dev(g["g_cov"]))
        got = dict(scales=s, rotations=r, opacities=o, reg=reg, d_scaling=ta.grad, d_rotation=tq.grad, d_opacity=tx.grad, cov=cov,
                   cov_d_scaling=ca.grad, cov_d_rotation=cq.grad)
        row = {"N": N, "fields": {}}
        for name, (truth, stated, scale) in fields.items():
            d = host(got[name]).reshape(np.asarray(stated).shape)
            e_dev = R.max_error(d, truth, scale)
            e_ref = max(R.max_error(stated, truth, scale), R.PARITY_FLOOR)
            row["fields"][name] = {"device_error": e_dev, "float32_statement_error_floored": e_ref, "ratio": round(e_dev / e_ref, 4),
                                   "bits_equal_float32_statement": bool(R.same_class_and_bits(d, stated))}
        row["largest_ratio"] = max(f["ratio"] for f in row["fields"].values())
        rows.append(row)
        print(json.dumps({"N": N, "largest_ratio": row["largest_ratio"],
                          "all_bits_equal_but_reg": all(f["bits_equal_float32_statement"] for k, f in row["fields"].items() if k != "reg")}), flush=True)
    out = {"metric": "max |device - float64 statement| / scale per field, over every element; ratio to the float32 statement's own error "
                     "(floored at 2^-24); the tests bound the ratio by 4",
           "device": torch.cuda.get_device_name(0), "epsilon": EPS, "scale_modifier": MOD,
           "inputs": "scaling in [-12, 4], quaternions of norm 1e-3 .. 1e3, logits in [-12, 12], upstream gradients of order one",
           "largest_ratio": max(r["largest_ratio"] for r in rows), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
