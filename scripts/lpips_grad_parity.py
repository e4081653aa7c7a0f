#!/usr/bin/env python3
"""The LPIPS backward's measured error per test case, in the unit tests/test_lpips_grad_gpu.py bounds it in:

    ratio = max|hip - f64| / max( max|f32 - f64|, 2^-23 max|f64| )          (the tests' bound is ratio <= 4)

f64 and f32 are tests/lpips_grad_ref.py's two modes (the float64 statement and the same loops in float32) on the same inputs: the head's
backward alone for wrt = 1, 2, 3, the transposed weights through conv3x3, and the whole chain at the tests' sizes GIVEN the activations
that the GPU forward stored.  The cases are the tests' own (tests/lpips_grad_cases.py, imported, not restated).

"host_statement_vs_autograd" needs no GPU: the float64 statement against torch's CPU float64 autograd at the sizes of
tests/test_lpips_grad_host.py, as worst |difference| / max |gradient|; that test's bound is 16 x the value recorded here.

Writes profiles/lpips_grad_parity.json (or --out) and prints one JSON summary line.  --host-only writes the host section alone (the
device sections of an existing file are kept).  Usage: python scripts/lpips_grad_parity.py [--out FILE] [--host-only]"""
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

import lpips_grad_cases as T  # noqa: E402
import test_lpips_grad_host as H  # noqa: E402


def row(e, y):
    return {"max_abs_err": e, "yardstick": y, "ratio": round(e / y, 3) if y else 0.0}


def host():
    out = {}
    for size in ((16, 16), (17, 31)):
        diff, scale, _ = H.statement_vs_autograd(size)
        out[f"{size[0]}x{size[1]}"] = {"max_abs_diff": diff, "max_abs_grad": scale, "relative": diff / scale}
    worst = max(v["relative"] for v in out.values())
    return {"what": "float64 statement against torch CPU float64 autograd, widths %s, two pairs" % (H.SMALL_WIDTHS,), "cases": out,
            "worst_relative": worst, "test_bound": H.AUTOGRAD_BOUND, "test_bound_over_worst": round(H.AUTOGRAD_BOUND / worst, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_grad_parity.json"))
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.out):
        out = json.load(open(a.out))
    out["host_statement_vs_autograd"] = host()
    summary = {"parity": "lpips_grad", "host_worst_relative": out["host_statement_vs_autograd"]["worst_relative"]}
    if not a.host_only:
        if not torch.cuda.is_available():
            raise SystemExit("lpips_grad_parity.py needs an MI355X (or --host-only)")
        head = {}
        for i, case in enumerate(T.HEAD_BWD_CASES):
            head[T.head_id(case)] = {f"wrt={wrt}": row(*T.measure_head_backward(i, wrt)) for wrt in (1, 2, 3)}
        convt = {"%d->%d, %dx%dx%d" % c: row(*T.measure_convt(i)) for i, c in enumerate(T.CONVT_CASES)}
        chain = {}
        for size in T.CHAIN_SIZES:
            chain["%dx%d" % size] = {f"wrt={wrt} d {which}": row(e, y) for wrt in (1, 2, 3) for which, e, y in T.measure_chain(size, wrt)}
        gates = {}
        for n in T.GATE_COUNTS:
            g, y, want = T.gate_case(n)
            gates[str(n)] = bool(np.array_equal(T.run_gate(g, y).cpu().numpy().view(np.int32), want.view(np.int32)))
        ratios = [r["ratio"] for group in (head, chain) for v in group.values() for r in v.values()] + [r["ratio"] for r in convt.values()]
        out.update({"metric": "ratio = max|hip - f64| over max(max|f32 - f64|, 2^-23 max|f64|); tests/test_lpips_grad_gpu.py requires <= 4 for "
                              "every compared map; all three evaluations take the activations of the GPU forward",
                    "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__, "precision": "fp32",
                    "bound": T.BOUND, "worst_ratio": max(ratios),
                    "head backward (P x C x h x w)": head, "gate bit-exact (element count)": gates,
                    "transposed weights through conv3x3 (Cin->Cout, B x H x W of the forward)": convt,
                    "whole chain (real widths, P = 2, normalize=True)": chain})
        summary["worst_ratio"] = out["worst_ratio"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
