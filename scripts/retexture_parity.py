#!/usr/bin/env python3
"""The retexture stage against its numpy statement (tests/retexture_ref.py) on an MI355X -> profiles/retexture_parity.json:

  cross     per (r, R) pair, mode and channel order: the number of float32 words whose bits differ from the statement's (a NaN on both
            sides counts as equal), expected 0; the golden case against the reference's own change_texture results as well.
  latlong   per case, picture type and mode: the largest error of the device against the float64 statement, the mixed-precision
            statement's own, and their ratio (the tests' bound is 4).

Usage: python scripts/retexture_parity.py [--out FILE]"""
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

import retexture_ref as R  # noqa: E402
from texgs import retexture  # noqa: E402

DEV = "cuda:0"
PAIRS = [(12, 12), (7, 5), (3, 8), (1, 4), (5, 33), (40, 17), (300, 1024)]
LATLONG_CASES = [(4, 8, 3), (16, 32, 8), (5, 7, 6), (64, 128, 33), (512, 1024, 256)]


def differing_words(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return int(((got.view(np.uint32) != want.view(np.uint32)) & ~both_nan).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retexture_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retexture_parity.py needs an MI355X")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)       # noqa: E731
    cross_rows, latlong_rows = [], []
    for r, R_ in PAIRS:
        cross, tex = R.hard_cross(r, seed=100 + r), R.hard_texture(R_, seed=200 + R_)
        new = {o: R.new01_of_u8(R.cross_new_u8(cross if o == "rgb" else cross[..., ::-1].copy(), R_, o)) for o in ("rgb", "bgr")}
        for mode in R.MODES:
            for order in ("rgb", "bgr"):
                src = cross if order == "rgb" else cross[..., ::-1]
                got = retexture.retexture_cross_u8(dev(tex), dev(src), mode=mode, order=order).cpu().numpy()
                want = R.mode_tail(tex, new[order], mode)
                cross_rows.append({"r": r, "R": R_, "mode": mode, "order": order, "words": int(got.size), "differing_words": differing_words(got, want),
                                   "nan_words": int(np.isnan(want).sum()), "inf_words": int(np.isinf(want).sum())})
    G = np.load(os.path.join(ROOT, "tests", "golden", "texture_io.npz"))
    golden = []
    for mode in R.MODES:
        got = retexture.retexture_cross_u8(dev(G["texture0"]), dev(G["cross_u8"]), mode=mode).cpu().numpy()
        golden.append({"mode": mode, "differing_words": differing_words(got, G[f"change_texture_m{mode + 1}"])})
    for h, w, R_ in LATLONG_CASES:
        for u8 in (False, True):
            rng = np.random.default_rng(1000 * h + R_)
            pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if u8 else rng.random((h, w, 3)).astype(np.float32)
            tex = rng.uniform(-1.5, 1.5, (6, R_, R_, 3)).astype(np.float32)
            for mode in (-1, 0):
                truth = R.latlong_f64(pic, R_, tex, mode)
                mixed = R.latlong_mixed(pic, R_, tex, mode)
                got = retexture.retexture_latlong(dev(pic), texture_sh0=None if mode == -1 else dev(tex), R=R_, mode=mode).cpu().numpy()
                e_dev, e_ref = float(np.abs(got.astype(np.float64) - truth).max()), float(np.abs(mixed.astype(np.float64) - truth).max())
                latlong_rows.append({"h": h, "w": w, "R": R_, "picture": "uint8" if u8 else "float32", "mode": mode, "device_error": e_dev,
                                     "mixed_statement_error": e_ref, "ratio": e_dev / e_ref, "differing_words_against_the_mixed_statement":
                                     differing_words(got, mixed), "words": int(got.size)})
    out = {"device": torch.cuda.get_device_name(0), "cross_differing_words_total": sum(r["differing_words"] for r in cross_rows),
           "golden_differing_words_total": sum(r["differing_words"] for r in golden),
           "latlong_worst_ratio": max(r["ratio"] for r in latlong_rows), "bound": 4.0, "golden": golden, "cross": cross_rows, "latlong": latlong_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("cross", "latlong", "golden")}), flush=True)


if __name__ == "__main__":
    main()
