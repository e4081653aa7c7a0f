#!/usr/bin/env python3
"""The UV-net kernels (csrc/uvnet.hip) on the device against the statement of tests/uvnet_ref.py, measured: the figures that
tests/test_uvnet_rows_gpu.py asserts on, for every case of it.

Forward, per probe / net, size and precision: the largest row error of uvs and of J against float64 over ALL rows (max |difference| of a
row / max |reference| of the row) and the row it is at, the float32 statement's own (its normalise step alone where the matrix
products are exact, the whole statement with the precision's split planes elsewhere; floored at 2^-24), their ratio, whether the rows
past N kept their fill, and the bit identities between the precisions.  Backward, per net, size and precision: per output the largest
entry error in units of the entry's scale and the entry it is at, the float32 statement's, the ratio of the largest to the statement's
largest; per point position of a tile the same for the one point's contribution and the count of entries that are zero in float64
but not on the device; NULL inputs and outputs.  The tests bound every ratio by 4.

Writes profiles/uvnet_rows_parity.json (or --out) and prints one JSON line per case.
Usage: python scripts/uvnet_rows_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import uvnet_ref as R  # noqa: E402
import test_uvnet_rows_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uvnet_rows_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uvnet_rows_parity.py needs an MI355X: there is no CPU path")
    out = {"probe_forward": [], "random_forward": [], "ragged_J": [], "backward": [], "position_sweep": [], "null_handling": []}

    def add(key, fig, brief):
        out[key].append(fig)
        print(json.dumps({"case": key, **{k: fig[k] for k in brief if k in fig}}), flush=True)

    for kind in R.PROBE_KINDS:
        for bias in (True, False):
            for norm in (True, False):
                for n in T.PROBE_SIZES:
                    add("probe_forward", T.figures_probe_forward(kind, bias, norm, n), ("probe", "bias", "norm", "N", "largest_ratio", "bit_identities"))
    for which in ("fresh", "golden", "rescaled"):
        for n in (33, 200):
            add("random_forward", T.figures_random_forward(which, n), ("net", "N", "largest_ratio", "bit_identities"))
    for prec in T.PRECISIONS:
        add("ragged_J", T.figures_ragged_J(prec), ("precision", "largest_ratio"))
    for which in ("probeA", "fresh", "rescaled"):
        for n in T.BACKWARD_SIZES:
            for prec in T.PRECISIONS:
                add("backward", T.figures_backward(which, n, prec), ("net", "N", "precision", "worst_output", "device_error", "float32_statement_error_floored",
                                                                       "ratio", "guards_untouched", "repeat_is_bit_identical"))
    for which in ("probeA", "fresh"):
        for prec in ("fp32", "mixed"):
            for n, pos in ((64, list(range(64))), (16_448, list(T.SWEEP_TAIL))):
                add("position_sweep", T.figures_position_sweep(which, prec, n, pos), ("net", "precision", "N", "largest_ratio"))
    for prec in ("fp32", "mixed"):
        add("null_handling", T.figures_null_handling(prec), ("precision", "guards_untouched", "null_inputs_equal_zero_bias_unit_scale", "null_output"))

    ratios = [f["largest_ratio"] for k in ("probe_forward", "random_forward", "ragged_J", "position_sweep") for f in out[k]] + [f["ratio"] for f in out["backward"]]
    identities = [v for k in ("probe_forward", "random_forward") for f in out[k] for v in f["bit_identities"].values()]
    summary = {
        "metric": "forward: per row max |device - float64| / max |float64| of the row, over all rows; backward: per entry |device - float64| / scale "
                  "of the entry (tests/uvnet_ref.backward); ratio to the float32 statement's own figure (floored at 2^-24); the tests bound every ratio by 4",
        "device": torch.cuda.get_device_name(0),
        "largest_ratio": max(ratios),
        "all_bit_identities": all(identities), "bit_identities_checked": len(identities),
        "probe_A_precisions_bit_identical": all(all(f["bit_identities"].values()) and len(f["bit_identities"]) == 6 for f in out["probe_forward"] if f["probe"] == "A"),
        "all_rows_past_N_untouched": all(p["rows_past_N_untouched"] for k in ("probe_forward", "random_forward") for f in out[k] for p in f["precision"].values())
        and all(s["rows_past_N_untouched"] for f in out["ragged_J"] for s in f["subsets"]),
        "all_guards_untouched": all(f["guards_untouched"] for f in out["backward"] + out["null_handling"]) and all(p["guards_untouched"] for f in out["position_sweep"] for p in f["positions"]),
        "all_repeats_bit_identical": all(f["repeat_is_bit_identical"] for f in out["backward"]),
        "nonzero_where_float64_is_zero": sum(p["nonzero_where_float64_is_zero"] for f in out["position_sweep"] for p in f["positions"]),
        "null_handling_ok": all(f["null_inputs_equal_zero_bias_unit_scale"] and all(f["null_output"].values()) for f in out["null_handling"]),
    }
    summary["largest_ratio"] = _sig(summary["largest_ratio"])
    summary["triples"] = "[device error, float32 statement's error floored at 2^-24, ratio, row or entry of the device's largest error]"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:          # one case per line
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in summary.items()))
        tables = {k: [_row(k, fig) for fig in figs] for k, figs in out.items()}
        f.write(",\n".join(f" {json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]" for k, rows in tables.items()))
        f.write("\n}\n")
    print(json.dumps(summary), flush=True)


def _sig(x):
    return float(f"{x:.4g}")


def _triple(f, where="worst_row"):
    return [_sig(f["device_error"]), _sig(f["float32_statement_error_floored"]), _sig(f["ratio"]), f[where]]


def _row(key, fig):
    """A case of the record on one line: what the tests assert on, figures to four digits."""
    if key in ("probe_forward", "random_forward"):
        row = {k: fig[k] for k in ("probe", "bias", "norm", "net", "N") if k in fig}
        for prec, f in fig["precision"].items():
            row[prec] = {"uvs": _triple(f["uvs"]), "J": _triple(f["J"])}
        if key == "probe_forward":          # where the statement says the matrix products are exact, the yardstick is the normalise step alone
            row["inexact_products"] = [f"{p}.{k}" for p, f in fig["precision"].items() for k in ("uvs", "J") if not f[k]["exact_products"]]
        return {**row, "rows_past_N_untouched": all(f["rows_past_N_untouched"] for f in fig["precision"].values()),
                "bit_identities_hold": sorted(k for k, v in fig["bit_identities"].items() if v),
                "bit_identities_broken": sorted(k for k, v in fig["bit_identities"].items() if not v), "largest_ratio": _sig(fig["largest_ratio"])}
    if key == "ragged_J":
        return {"precision": fig["precision"], "largest_ratio": _sig(fig["largest_ratio"]),
                "rows_past_N_untouched": all(s["rows_past_N_untouched"] for s in fig["subsets"]),
                "subsets": {f"{s['rows'][0]}:{s['rows'][1]}": _triple(s) for s in fig["subsets"]}}
    if key == "backward":
        worst = fig["outputs"][fig["worst_output"]]
        return {**{k: fig[k] for k in ("net", "N", "precision", "worst_output")}, "worst_entry": worst["worst_entry"],
                "device_error": _sig(fig["device_error"]), "float32_statement_error_floored": _sig(fig["float32_statement_error_floored"]),
                "ratio": _sig(fig["ratio"]), "device_error_per_output": {k: _sig(v["device_error"]) for k, v in fig["outputs"].items()},
                "guards_untouched": fig["guards_untouched"], "repeat_is_bit_identical": fig["repeat_is_bit_identical"]}
    if key == "position_sweep":
        pos = fig["positions"]
        worst = max(pos, key=lambda p: p["ratio"])
        return {**{k: fig[k] for k in ("net", "precision", "N")}, "positions": [pos[0]["p"], pos[-1]["p"]],
                "float32_statement_error_floored_min_max": [_sig(min(p["float32_statement_error_floored"] for p in pos)),
                                                            _sig(max(p["float32_statement_error_floored"] for p in pos))],
                "largest_ratio": _sig(fig["largest_ratio"]),
                "worst_position": worst["p"], "worst_output": worst["worst_output"], "worst_entry": worst["worst_entry"],
                "smallest_ratio": _sig(min(p["ratio"] for p in pos)), "guards_untouched": all(p["guards_untouched"] for p in pos),
                "float64_zero_entries_at_least": min(p["float64_zero_entries"] for p in pos),
                "nonzero_where_float64_is_zero": sum(p["nonzero_where_float64_is_zero"] for p in pos)}
    return fig


if __name__ == "__main__":
    main()
