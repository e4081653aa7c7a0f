#!/usr/bin/env python3
"""The measured maxima behind the tolerances of tests/test_density_gpu.py: texgs.density on the GPU against the reference's own
results (tests/golden/density.npz) and against the numpy statement (tests/density_ref.py).  Bounds: children's xyz and scaling 2e-6
absolute, accumulated norms 1e-6 relative; everything else is compared for equality by the tests.
Writes profiles/density_parity.json (or --out).  Usage: python scripts/density_parity.py [--out FILE]"""
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

import density_ref as R  # noqa: E402
from texgs import density  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def model(params_np, moments=None):
    params = {k: torch.nn.Parameter(dev(params_np[k])) for k in R.GROUPS}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-4, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    if moments is not None:
        for k, p in params.items():
            opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": dev(moments[k][0]), "exp_avg_sq": dev(moments[k][1])}
    return params, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_parity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_parity.py needs an MI355X")
    G = R.golden()
    out = {"device": torch.cuda.get_device_name(0), "bounds": {"children_abs": R.TOL_CHILD, "norms_rel": R.TOL_NORM}, "golden": {}, "statement": {}}
    for tag in ("sh3", "sh1"):
        params_np, moments, accum, denom = R.golden_case(tag)
        params, opt = model(params_np, moments)
        st = density.DensityState(dev(accum), dev(denom), dev(G[f"{tag}_in_max_radii2D"]))
        max_grad, min_opacity, extent, mss, pd = (float(v) for v in G[f"{tag}_settings"])
        new = density.densify_and_prune(params, opt, st, max_grad=max_grad, min_opacity=min_opacity, extent=extent, max_screen_size=mss or None,
                                        percent_dense=pd, noise=dev(G[f"{tag}_eps"]))
        m = G[f"{tag}_out_xyz"].shape[0]
        first_child = m - 2 * int(G[f"{tag}_class_counts"][2])
        row = {"rows": [int(accum.shape[0]), int(new["xyz"].shape[0])], "rows_reference": int(m)}
        for k in ("xyz", "scaling"):
            got = new[k].detach().cpu().numpy().astype(np.float64)
            row[f"children_{k}_max_abs"] = float(np.abs(got[first_child:] - G[f"{tag}_out_{k}"][first_child:]).max())
            row[f"copied_{k}_equal"] = bool(np.array_equal(got[:first_child], G[f"{tag}_out_{k}"][:first_child].astype(np.float64)))
        out["golden"][tag] = row
    st = density.DensityState.zeros(G["stats_radii0"].shape[0], "cuda")
    for r in range(2):
        density.add_densification_stats(st, dev(G[f"stats_grad{r}"]), dev(G[f"stats_radii{r}"]))
        want = G[f"stats_accum{r}"].astype(np.float64)
        rel = np.abs(st.xyz_gradient_accum.cpu().numpy().astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
        out["golden"][f"stats_round{r}_norms_max_rel"] = float(rel.max())
    n = G["reset_in_opacity"].shape[0]
    p_np = R.cloud(n, 1, width_rest=9)[0]
    p_np["opacity"] = G["reset_in_opacity"]
    params, opt = model(p_np)
    got = density.reset_opacity(params, opt).detach().cpu().numpy().astype(np.float64)
    out["golden"]["reset_opacity_max_abs"] = float(np.abs(got - G["reset_out_opacity"]).max())
    # against the numpy statement at a size with several blocks
    kw = dict(max_grad=0.0002, min_opacity=0.005, dense_scale=0.01, big_scale=0.1)
    for width in (45, 9):
        n = 100003
        p_np, accum, denom, noise = R.cloud(n, 7 + width, width_rest=width, frac=(0.2, 0.2, 0.1))
        action, rank, totals = R.plan_np(accum, denom, p_np["scaling"], p_np["opacity"], **kw)
        noise = noise[:2 * totals[2]]
        want, _ = R.move_np(p_np, {}, action, rank, totals, noise)
        params, opt = model(p_np)
        st = density.DensityState(dev(accum), dev(denom), torch.zeros(n, device="cuda"))
        new = density.densify_and_prune(params, opt, st, max_grad=kw["max_grad"], min_opacity=kw["min_opacity"], extent=1.0, max_screen_size=20,
                                        percent_dense=0.01, noise=dev(noise))
        c = int(totals[0] + totals[1])
        row = {"N": n, "rows_after": int(new["xyz"].shape[0]), "rows_statement": int(want["xyz"].shape[0])}
        for k in ("xyz", "scaling"):
            got = new[k].detach().cpu().numpy()
            row[f"children_{k}_max_abs"] = float(np.abs(got[c:].astype(np.float64) - want[k][c:]).max())
            row[f"copied_{k}_equal"] = bool(np.array_equal(got[:c], want[k][:c]))
        row["other_tensors_equal"] = all(np.array_equal(new[k].detach().cpu().numpy(), want[k]) for k in ("f_dc", "f_rest", "opacity", "rotation"))
        out["statement"][f"f_rest_width_{width}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
