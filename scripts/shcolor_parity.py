#!/usr/bin/env python3
"""The colour stage on the device against the numpy statements of tests/shcolor_ref.py, measured: for every (degree, max degree)
pair and size, whether the forward's bits equal the float32 statement's (sh_colors on one tensor and on the (dc, rest) pair, eval_sh
on the transposed view), and for the backward the error against the float64 statement (max |device - float64| / scale over every
element, the scales of shcolor_ref.backward_scales), the float32 statement's own error floored at 2^-24, their ratio (the tests bound
it by 4) and whether the bits are the statement's; the same for 1, 3 and 17 views at degree 3.

Writes profiles/shcolor_parity.json (or --out) and prints one JSON line per row.
Usage: python scripts/shcolor_parity.py [--sizes 1,65,...] [--out FILE]"""
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

import shcolor_ref as R  # noqa: E402
from texgs import shcolor as S  # noqa: E402

DEV = "cuda:0"


def main():
    rpw = S.ROWS_PER_WORKGROUP
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(n) for n in (1, 65, rpw, rpw + 1, 1000, 20001)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shcolor_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shcolor_parity.py needs an MI355X: there is no CPU path")
    dev = lambda v, grad=False: torch.tensor(np.asarray(v, R.F), device=DEV).requires_grad_(grad)       # noqa: E731
    host = lambda t: t.detach().cpu().numpy()       # noqa: E731
    bits = lambda a, b: bool(R.same_class_and_bits(np.asarray(a), np.asarray(b).reshape(np.asarray(a).shape)))      # noqa: E731
    rows = []

    def measure(deg, K, N, V):
        sh, xyz, cams, g = R.random_case(N, K, 7 + 1000 * K + N, V)
        feats, tx = dev(sh, True), dev(xyz, True)
        cols = S.sh_colors_views(feats, tx, dev(cams), deg)
        (cols * dev(g)).sum().backward()
        want = R.S32.colors_views(deg, sh, xyz, cams)
        with torch.no_grad():
            pair = S.sh_colors_views((dev(sh[:, :1]), dev(sh[:, 1:])), dev(xyz), dev(cams), deg)
            d = R.S32.direction(xyz, cams[0])[0] if deg else np.zeros_like(xyz)
            ev = S.eval_sh(deg, dev(sh).transpose(1, 2), dev(d))
        row = {"degree": deg, "K": K, "N": N, "views": V, "clamped_fraction": round(float((want == 0).mean()), 4),
               "forward_bits_equal": {"sh_colors": bits(host(cols), want), "pair": bits(host(pair), want),
                                      "eval_sh_transposed_view": bits(host(ev), R.S32.eval_sh(deg, sh, d))}, "backward": {}}
        truth = R.S64.colors_backward(deg, sh, xyz, cams, g)
        stated = R.S32.colors_backward(deg, sh, xyz, cams, g)
        scales = R.backward_scales(deg, sh, xyz, cams, g)
        for name, got, t, s, sc in zip(("d_features", "d_xyz"), (host(feats.grad), host(tx.grad)), truth, stated, scales):
            e_dev = R.max_error(got, t, sc)
            e_ref = max(R.max_error(s, t, sc), R.PARITY_FLOOR)
            row["backward"][name] = {"device_error": e_dev, "float32_statement_error_floored": e_ref, "ratio": round(e_dev / e_ref, 4),
                                     "bits_equal_float32_statement": bits(got, s)}
        row["largest_ratio"] = max(f["ratio"] for f in row["backward"].values())
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("degree", "K", "N", "views", "forward_bits_equal", "largest_ratio")}), flush=True)

    for mx in range(5):
        for deg in range(mx + 1):
            for N in [int(s) for s in args.sizes.split(",")]:
                measure(deg, (mx + 1) ** 2, N, 1)
    for V in (3, 17):
        measure(3, 16, 2 * rpw + 1, V)
    out = {"metric": "forward: bits equal to the float32 statement; backward: max |device - float64 statement| / scale per field over "
                     "every element, ratio to the float32 statement's own error (floored at 2^-24); the tests bound the ratio by 4",
           "device": torch.cuda.get_device_name(0),
           "inputs": "standard-normal coefficients, points 2 to 6 units from cameras within a unit of the origin, upstream gradients of order one",
           "all_forward_bits_equal": all(all(r["forward_bits_equal"].values()) for r in rows),
           "all_backward_bits_equal": all(f["bits_equal_float32_statement"] for r in rows for f in r["backward"].values()),
           "largest_ratio": max(r["largest_ratio"] for r in rows), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
