#!/usr/bin/env python3
"""The parameter stage two ways, timed in the same process, at N = 300 000 and 1 000 000:

  stage       the stage alone, forward + backward with the regulariser: texgs.params.activate(..., opacity_reg=True) (two launches
              forward, one backward) against the torch composition the reference executes under autograd (exp, F.normalize, sigmoid,
              texgs.losses.zero_one_loss).  The same four upstream gradients go into both.
  iteration   two renders of one texgs.synth view (sh_degree 3, then 0) plus one backward, the reference's pattern: one side
              activates with torch inside each render (the getters run per render() call), the other calls texgs.params.activate
              once and hands the same tensors to both renders.

Host wall clock around work that ends synchronised, the two legs alternating inside one loop; medians with p10-p90 of --reps
repetitions.  verdict: "faster" / "slower" when the medians differ by more than the TORCH leg's own p10-p90 spread, "tie" inside it.
The two legs' results are compared in this run (largest relative difference); the bit-exact comparison is the test suite's.

Writes profiles/params_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_params.py [--reps 30] [--warmup 4] [--sizes 300000,1000000] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import losses as LS, params, synth  # noqa: E402
from texgs.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_p90_ms": [round(float(np.percentile(v, q)), 4) for q in (10, 90)]}


def verdict(r, o):
    """Against the torch leg's own spread"""
    spread = r["p10_p90_ms"][1] - r["p10_p90_ms"][0]
    d = r["median_ms"] - o["median_ms"]
    return "tie" if abs(d) <= spread else ("faster" if d > 0 else "slower")


def alternate(ref, ours, reps, warmup):
    for _ in range(warmup):
        ref(), ours()
    t_ref, t_ours = [], []
    for _ in range(reps):
        t_ref.append(wall_ms(ref))
        t_ours.append(wall_ms(ours))
    r, o = stats(t_ref), stats(t_ours)
    return {"torch": r, "params": o, "torch_minus_params_ms": round(r["median_ms"] - o["median_ms"], 4),
            "torch_over_params": round(r["median_ms"] / o["median_ms"], 3), "verdict": verdict(r, o)}


def norm_diff(a, b):
    """Relative L2 difference (an element-wise ratio would measure the cancellation in g - r (r . g), not the legs)"""
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions per row")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sizes", default="300000,1000000")
    ap.add_argument("--res", type=int, default=1024, help="texture resolution of the synthetic scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_params.py needs an MI355X: there is no CPU path to time")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    W = H = 800
    for N in [int(s) for s in args.sizes.split(",")]:
        scene = synth.make_scene(N, args.res, seed=0)
        cam = synth.fibonacci_cameras(64, W, H)[5]
        P = lambda t: t.float().to(DEV).contiguous().requires_grad_(True)         # noqa: E731
        raw = dict(scaling=P(scene.scales.log()), rotation=P(scene.rotations * (0.5 + torch.rand(N, 1))),
                   opacity=P(torch.logit(scene.opacities.clamp(1e-6, 1 - 1e-6))))
        leaves = list(raw.values())

        def drop_grads():
            for t in leaves:
                t.grad = None

        # ---- the stage alone ----
        g = torch.Generator().manual_seed(3)
        ups = [torch.randn(N, 3, generator=g).to(DEV), torch.randn(N, 4, generator=g).to(DEV), torch.randn(N, 1, generator=g).to(DEV),
               torch.tensor(0.001, device=DEV)]

        def stage_torch(keep=False):
            s, r, o = torch.exp(raw["scaling"]), F.normalize(raw["rotation"]), torch.sigmoid(raw["opacity"])
            reg = LS.zero_one_loss(o)
            torch.autograd.backward([s, r, o, reg], ups)
            out = [t.grad for t in leaves] + [reg.detach()]
            if not keep:
                drop_grads()
            return out

        def stage_hip(keep=False):
            s, r, o, reg = params.activate(raw["scaling"], raw["rotation"], raw["opacity"], opacity_reg=True)
            torch.autograd.backward([s, r, o, reg], ups)
            out = [t.grad for t in leaves] + [reg.detach()]
            if not keep:
                drop_grads()
            return out

        a = stage_torch(keep=True); drop_grads()
        b = stage_hip(keep=True); drop_grads()
        row = {"row": "stage", "N": N, "params_launches": 3,
               "relative_l2_difference_between_legs": {k: norm_diff(x, y) for k, x, y in zip(("d_scaling", "d_rotation", "d_opacity", "reg"), b, a)}}
        row.update(alternate(stage_torch, stage_hip, args.reps, args.warmup))
        emit(row)

        # ---- two renders and one backward ----
        f = lambda t: t.float().to(DEV).contiguous()        # noqa: E731
        cam_t = dict(viewmatrix=f(cam.world_view_transform), projmatrix=f(cam.full_proj_transform), campos=f(cam.camera_center))
        st3 = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                            bg=torch.zeros(3, device=DEV), scale_modifier=1.0, sh_degree=3, prefiltered=False, debug=False,
                                            **cam_t)
        st0 = st3._replace(sh_degree=0)
        fixed = dict(means3D=f(scene.means3D), shs=f(scene.shs), uvs=f(scene.uvs), gradient_uvs=f(scene.gradient_uvs), texture=f(scene.texture))
        w3, w0 = torch.rand(3, H, W, generator=g).to(DEV), torch.rand(3, H, W, generator=g).to(DEV)

        def render(st, s, r, o):
            return GaussianRasterizer(st)(means3D=fixed["means3D"], means2D=torch.zeros_like(fixed["means3D"]), shs=fixed["shs"], opacities=o,
                                          scales=s, rotations=r, uvs=fixed["uvs"], gradient_uvs=fixed["gradient_uvs"], texture=fixed["texture"],
                                          extra_attrs=None)[0]

        def iter_torch(keep=False):         # the getters run per render() call
            act = lambda: (torch.exp(raw["scaling"]), F.normalize(raw["rotation"]), torch.sigmoid(raw["opacity"]))        # noqa: E731
            loss = (render(st3, *act()) * w3).sum() + 2.0 * (render(st0, *act()) * w0).sum()
            loss.backward()
            out = [t.grad for t in leaves]
            if not keep:
                drop_grads()
            return out

        def iter_hip(keep=False):           # once per iteration, shared by both renders
            s, r, o = params.activate(raw["scaling"], raw["rotation"], raw["opacity"])
            loss = (render(st3, s, r, o) * w3).sum() + 2.0 * (render(st0, s, r, o) * w0).sum()
            loss.backward()
            out = [t.grad for t in leaves]
            if not keep:
                drop_grads()
            return out

        a = iter_torch(keep=True); drop_grads()
        b = iter_hip(keep=True); drop_grads()
        row = {"row": "iteration", "N": N, "image": [H, W], "texture_res": args.res,
               "relative_l2_difference_between_legs": {k: norm_diff(x, y) for k, x, y in zip(("d_scaling", "d_rotation", "d_opacity"), b, a)}}
        row.update(alternate(iter_torch, iter_hip, args.reps, args.warmup))
        emit(row)
        del scene, raw, leaves, fixed, ups, w3, w0
        torch.cuda.empty_cache()

    out = {"metric": "host wall-clock ms of work that ends synchronised; medians and p10-p90 of alternating repetitions in one process; "
                     "verdict against the torch leg's own p10-p90 spread",
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "reps": args.reps, "warmup": args.warmup,
           "slower_rows": [{"row": r["row"], "N": r["N"]} for r in rows if r.get("verdict") == "slower"],
           "tied_rows": [{"row": r["row"], "N": r["N"]} for r in rows if r.get("verdict") == "tie"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
