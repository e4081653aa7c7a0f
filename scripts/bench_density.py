#!/usr/bin/env python3
"""Stage-1 density control (texgs.density, csrc/density.hip) against the reference's statement of the same two steps written with
torch operations on the same GPU tensors, timed in the same process:

  stats     the per-step statistics: one launch against the three boolean-mask updates of models/gaussian3d.py:431-432, :334-336
  densify   one densify_and_prune with about 5 % cloned, 5 % split and 3 % pruned: plan + one move against the reference's
            cat / cat / mask / mask of the six parameters and both Adam moments (:200-332, restated below; no empty_cache)

N = 300 000 and 1 000 000, SH degree 3 (59 floats per Gaussian, x 3 with the moments).  Every shape is warmed up on both sides;
the timed calls alternate hip / torch; a timing is a pair of device events around one call inside a synchronised window (the
densify call holds one readback on either side: the totals here, nonzero / mask sums there).  The model is rebuilt outside the
window before every densify call.  Both sides must produce the same number of rows.

Bytes: the move's floor is one read and one write of 59 x 3 floats per surviving row (1416 B); `floor_GBps` is that over the
fused call's time, plan and readback included.

Writes profiles/density_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_density.py [--reps 7] [--quick] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import density  # noqa: E402

GROUPS = density.GROUPS
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
FLOATS = sum(int(np.prod(s)) for s in SHAPES.values())          # 59
KW = dict(max_grad=0.0002, min_opacity=0.005, extent=1.0, max_screen_size=20, percent_dense=0.01)


def make_cloud(n, dev, seed):
    """base tensors by name + moments + accum / denom: ~5 % small and hot (clone), ~5 % large and hot (split), ~3 % transparent"""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    u = torch.rand(n, generator=g, device=dev)
    clone, split, prune = u < 0.05, (u >= 0.05) & (u < 0.10), (u >= 0.10) & (u < 0.13)
    base = {k: rn(n, *s) for k, s in SHAPES.items()}
    base["scaling"] = torch.where(split[:, None], torch.full((n, 3), float(np.log(0.03)), device=dev), torch.full((n, 3), float(np.log(0.004)), device=dev)) \
        + 0.1 * rn(n, 3)
    base["opacity"] = torch.where(prune[:, None], torch.full((n, 1), -7.0, device=dev), 2.0 + 0.5 * rn(n, 1))
    mom = {k: (0.1 * rn(n, *s), (0.1 * rn(n, *s)).square()) for k, s in SHAPES.items()}
    denom = torch.randint(1, 6, (n, 1), generator=g, device=dev).float()
    grad = torch.where((clone | split)[:, None], torch.full((n, 1), 3 * KW["max_grad"], device=dev), torch.full((n, 1), 0.1 * KW["max_grad"], device=dev))
    return base, mom, grad * denom, denom


def make_model(base, mom, accum, denom):
    params = {k: nn.Parameter(base[k].clone()) for k in GROUPS}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-4, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for k, p in params.items():
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": mom[k][0].clone(), "exp_avg_sq": mom[k][1].clone()}
    st = density.DensityState(accum.clone(), denom.clone(), torch.zeros(accum.shape[0], device=accum.device))
    return params, opt, st


# ---- the reference's statement, torch operations on the same tensors (models/gaussian3d.py:200-336) ----
def torch_stats(st, grad, radii):
    vis = radii > 0
    st.max_radii2D[vis] = torch.max(st.max_radii2D[vis], radii[vis])
    st.xyz_gradient_accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
    st.denom[vis] += 1


def _cat(opt, params, new):
    for group in opt.param_groups:
        name, old = group["name"], group["params"][0]
        stored = opt.state.get(old)
        stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(new[name])), dim=0)
        stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(new[name])), dim=0)
        del opt.state[old]
        group["params"][0] = nn.Parameter(torch.cat((old, new[name]), dim=0).requires_grad_(True))
        opt.state[group["params"][0]] = stored
        params[name] = group["params"][0]


def _mask(opt, params, keep):
    for group in opt.param_groups:
        name, old = group["name"], group["params"][0]
        stored = opt.state.get(old)
        stored["exp_avg"] = stored["exp_avg"][keep]
        stored["exp_avg_sq"] = stored["exp_avg_sq"][keep]
        del opt.state[old]
        group["params"][0] = nn.Parameter(old[keep].requires_grad_(True))
        opt.state[group["params"][0]] = stored
        params[name] = group["params"][0]


def _rotation(r):
    q = r / torch.sqrt((r * r).sum(1))[:, None]
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_densify(params, opt, st, noise_gen):
    dev = params["xyz"].device
    grads = st.xyz_gradient_accum / st.denom
    grads[grads.isnan()] = 0.0
    dense = KW["percent_dense"] * KW["extent"]
    with torch.no_grad():
        sel = (torch.norm(grads, dim=-1) >= KW["max_grad"]) & (torch.exp(params["scaling"]).max(dim=1).values <= dense)
        _cat(opt, params, {k: params[k][sel] for k in GROUPS})
        n = params["xyz"].shape[0]
        padded = torch.zeros(n, device=dev)
        padded[:grads.shape[0]] = grads.squeeze()
        s = torch.exp(params["scaling"])
        sel = (padded >= KW["max_grad"]) & (s.max(dim=1).values > dense)
        stds = s[sel].repeat(2, 1)
        samples = stds * torch.randn(stds.shape, generator=noise_gen, device=dev)
        rots = _rotation(params["rotation"][sel]).repeat(2, 1, 1)
        new = {k: params[k][sel].repeat(2, *([1] * (params[k].dim() - 1))) for k in GROUPS}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + new["xyz"]
        new["scaling"] = torch.log(stds / 1.6)
        _cat(opt, params, new)
        _mask(opt, params, ~torch.cat((sel, torch.zeros(2 * int(sel.sum()), device=dev, dtype=torch.bool))))
        prune = (torch.sigmoid(params["opacity"]) < KW["min_opacity"]).squeeze()
        if KW["max_screen_size"]:
            prune = prune | (torch.exp(params["scaling"]).max(dim=1).values > 0.1 * KW["extent"])
        _mask(opt, params, ~prune)
    m = params["xyz"].shape[0]
    z = lambda *sh: torch.zeros(sh, device=dev)
    st.xyz_gradient_accum, st.denom, st.max_radii2D = z(m, 1), z(m, 1), z(m)
    return params


def event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="leave N = 1 M out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_density.py needs an MI355X; there is nothing to measure without one")
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 4)
    rows = []
    for n in [300_000] + ([] if args.quick else [1_000_000]):
        base, mom, accum, denom = make_cloud(n, dev, 1)
        g = torch.Generator(device=dev).manual_seed(2)
        grad = 1e-3 * torch.randn(n, 3, generator=g, device=dev)
        radii = (torch.randint(1, 40, (n,), generator=g, device=dev) * (torch.rand(n, generator=g, device=dev) < 0.4)).int()
        # statistics: 20 calls per event pair (one call is a few microseconds of device time)
        sts = [density.DensityState.zeros(n, dev) for _ in range(2)]
        hip = lambda: [density.add_densification_stats(sts[0], grad, radii) for _ in range(20)]
        ref = lambda: [torch_stats(sts[1], grad, radii) for _ in range(20)]
        event_ms(hip), event_ms(ref)
        same = all(torch.allclose(getattr(sts[0], k), getattr(sts[1], k), rtol=1e-6, atol=0) for k in ("xyz_gradient_accum", "denom", "max_radii2D"))
        t_hip, t_ref = [], []
        for _ in range(args.reps):
            t_hip.append(event_ms(hip)[0] / 20)
            t_ref.append(event_ms(ref)[0] / 20)
        row = {"op": "stats", "N": n, "hip_ms": med(t_hip), "torch_ms": med(t_ref), "hip_all_ms": [round(t, 4) for t in t_hip],
               "torch_all_ms": [round(t, 4) for t in t_ref], "results_agree": bool(same), "visible_share": round(float((radii > 0).float().mean()), 3)}
        row["speedup_vs_torch"] = round(row["torch_ms"] / row["hip_ms"], 2)
        row["hip_faster"] = row["hip_ms"] < row["torch_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        # densify_and_prune
        t_hip, t_ref, m_hip, m_ref, shares = [], [], None, None, None
        for i in range(args.reps + 1):                  # the first round is the warm-up
            params, opt, st = make_model(base, mom, accum, denom)
            if shares is None:
                act = density._plan_densify({k: params[k].detach() for k in ("scaling", "opacity")}, st, max_grad=KW["max_grad"],
                                           min_opacity=KW["min_opacity"], dense_scale=0.01, big_scale=0.1)[2].tolist()
                shares = {"kept": act[0] / n, "clone": act[1] / n, "split": act[2] / n, "children_kept": act[3] / n}
            ng = torch.Generator(device=dev).manual_seed(5)
            t, new = event_ms(lambda: density.densify_and_prune(params, opt, st, generator=ng, **KW))
            m_hip = new["xyz"].shape[0]
            del params, opt, st, new
            params, opt, st = make_model(base, mom, accum, denom)
            ng = torch.Generator(device=dev).manual_seed(5)
            t2, new = event_ms(lambda: torch_densify(params, opt, st, ng))
            m_ref = new["xyz"].shape[0]
            del params, opt, st, new
            if i:
                t_hip.append(t)
                t_ref.append(t2)
        floor = 2 * 3 * FLOATS * 4
        row = {"op": "densify_and_prune", "N": n, "rows_after": m_hip, "rows_after_torch": m_ref, "results_agree": m_hip == m_ref,
               "shares": {k: round(v, 4) for k, v in shares.items()}, "pruned_share": round(1 - shares["kept"] - shares["split"], 4),
               "hip_ms": med(t_hip), "torch_ms": med(t_ref), "hip_all_ms": [round(t, 4) for t in t_hip],
               "torch_all_ms": [round(t, 4) for t in t_ref], "floor_bytes_per_surviving_row": floor,
               "floor_GBps": round(floor * m_hip / (med(t_hip) * 1e-3) / 1e9, 1),
               "torch_GBps_same_bytes": round(floor * m_ref / (med(t_ref) * 1e-3) / 1e9, 1)}
        row["speedup_vs_torch"] = round(row["torch_ms"] / row["hip_ms"], 2)
        row["hip_faster"] = row["hip_ms"] < row["torch_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del base, mom, accum, denom
    out = {"metric": "texgs.density against the reference's statement in torch, device-event ms per call (median)",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "floats_per_gaussian": FLOATS, "rows": rows,
           "hip_faster_on_every_row": all(r["hip_faster"] for r in rows), "results_agree_on_every_row": all(r["results_agree"] for r in rows)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
