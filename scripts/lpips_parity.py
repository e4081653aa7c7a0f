#!/usr/bin/env python3
"""The LPIPS stage's measured error per test case, in the unit tests/test_lpips_gpu.py bounds it in:

    ratio = max|hip - f64| / max( max|f32 - f64|, 2^-23 max|f64| )          (the tests' bound is ratio <= 4)

f64 and f32 are tests/lpips_ref.py's two modes (the float64 statement and the same loops as a plain k-ordered fp32 chain) on the same
inputs: the convolution cases of the tests, the head cases, and the whole net at the tests' sizes -- the five tapped maps, the five
layers' terms and the value, with the absolute error of the value next to it (the metric is reported to three decimals).
The cases are the tests' own (tests/lpips_cases.py, imported, not restated).  Only precision "fp32" exists: "bf16x3" is not built.

Writes profiles/lpips_parity.json (or --out) and prints one JSON summary line.  Usage: python scripts/lpips_parity.py [--out FILE]"""
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

import lpips_ref as R  # noqa: E402
import lpips_cases as T  # noqa: E402


def ratio(got, f64, f32):
    err = float(np.abs(np.asarray(got, np.float64) - f64).max())
    return {"max_abs_err": err, "ratio": round(4 * err / R.tolerance(f64, f32), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_parity.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_parity.py needs an MI355X")
    conv = {}
    for k in range(T.N_CONV):
        c, d = T.conv_case(k)
        conv[f"{k:02d} {T.cid(c)}"] = ratio(T.run_conv(c, d).cpu().numpy(), d["y64"], d["y32"])
    head = {}
    for k, case in enumerate(T.HEAD_CASES):
        d = T.head_case(k)
        got = T.run_head(T.cuda(d["f"]), T.cuda(d["lin"]))[:, 0].cpu().numpy()
        rel = lambda v: float((np.abs(v - d["v64"]) / d["v64"]).max())
        head["x".join(map(str, case[:4])) + (f" {case[4]}" if case[4] else "")] = {"hip_rel_err": rel(got), "f32_statement_rel_err": rel(d["v32"])}
    net, _, _ = T.net()
    whole = {}
    for size in T.NET_SIZES:
        d = T.net_case(size)
        a0, a1 = T.cuda(d["img0"]), T.cuda(d["img1"])
        taps = net.features(torch.cat([a0, a1]), normalize=True)
        row = {f"relu{k + 1}": ratio(t.cpu().numpy(), d["taps64"][k], d["taps32"][k]) for k, t in enumerate(taps)}
        L = net.layers(a0, a1, normalize=True).cpu().numpy()
        row["layers"] = {"hip_abs_err": np.abs(L - d["layers64"]).max(axis=0).tolist(),
                         "f32_statement_abs_err": np.abs(d["layers32"] - d["layers64"]).max(axis=0).tolist()}
        v = net(a0, a1, normalize=True).cpu().numpy().reshape(-1).astype(np.float64)
        v64 = T.value(d["layers64"])
        row["value"] = {"lpips": v64.tolist(), "hip_abs_err": float(np.abs(v - v64).max()),
                        "f32_statement_abs_err": float(np.abs(T.value(d["layers32"]) - v64).max())}
        whole[f"{size[0]}x{size[1]}"] = row
    worst = max([v["ratio"] for v in conv.values()] + [v["ratio"] for r in whole.values() for k, v in r.items() if k.startswith("relu")])
    out = {"metric": "ratio = max|hip - f64| over max(max|f32 - f64|, 2^-23 max|f64|), tests/test_lpips_gpu.py requires <= 4 for every map; "
                     "scalars: the hip error next to the f32 statement's own, which the tests compare as maxima over all cases",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "precision": "fp32",
           "bf16x3": "not built: no measurement, no bound", "bound": 4, "worst_ratio": worst,
           "conv cases (B x Cin x Cout x H x W)": conv, "head cases (P x C x h x w)": head, "whole net (real widths, P = 2)": whole}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"parity": "lpips", "worst_ratio": worst, "lpips_abs_err_32x48": whole["32x48"]["value"]["hip_abs_err"]}))


if __name__ == "__main__":
    main()
