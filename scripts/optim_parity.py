#!/usr/bin/env python3
"""How far texgs.optim.FusedAdam lies from torch's own Adam on the same GPU, and how far torch's CPU Adam lies from it on the same
inputs (the reference's own spread): one-step differences in units of 2^-24 of a scale, measured by
tests/test_optim_gpu.py::measure_parity (65 536 elements, 8 steps, gradient magnitudes log-uniform in 1e-24 .. 1e2, every 7th zero).
The test's p' bound is twice the `ours` p' figure of seed 1 recorded here, and at most 16.

Writes profiles/optim_parity.json (or --out).  Usage: python scripts/optim_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_parity.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_parity.py needs an MI355X")
    import test_optim_gpu as T
    seeds = {str(seed): T.measure_parity(seed=seed) for seed in (1, 2, 3)}
    worst_p = max(r["ours"][0] for r in seeds["1"].values())
    out = {"metric": "worst one-step difference over 8 steps x 65536 elements, in units of 2^-24 of max(|p|, |p'-p|) for p', "
                     "max(|m|, |g|) for m', max(v, g^2) for v' (each floored at the smallest normal f32); [p', m', v']",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "ours": "texgs.optim.FusedAdam against the yardstick", "torch_cpu": "torch.optim.Adam on the CPU against the yardstick",
           "seeds": seeds, "p_measured_seed_1": worst_p, "p_bound_of_the_test": min(2.0 * worst_p, 16.0),
           "bounds": {"m": 4.0, "v": 4.0, "p_max": 16.0}}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"parity": "optim", "p_measured_seed_1": worst_p, "seeds": seeds}))


if __name__ == "__main__":
    main()
