#!/usr/bin/env python3
"""One stage-2 (UV-map) iteration on the C3 scene at 800x800 (models/uv_map_gaussian3d.py:167-232 with configs/uv_map.yaml's
weights: Linv, Lchamfer, Linv2; the uniform samples shared between the later terms), timed two ways in the same run:

  hip       texgs.uvmap: hash-grid encoding and its backward in HIP (csrc/uvmap.hip), chamfer nearest neighbours in HIP
  baseline  the same iteration with the float64 statement's fp32 twin: the grid as torch gathers (autograd's index backward
            = index_put_ / index_add_) and chamfer as torch.cdist + min

Prints one JSON line: the valid-point count, median ms per iteration over --steps timed iterations (after --warmup), and the
split render / uv fwd / inverse fwd (+ Linv) / chamfer (+ Linv2's uv fwd) / backward (HIP events between phases; phases are not synchronised, so the split
sums to the total).  The target point cloud is a random 16 384-point subset of the means (its content does not change the cost).
Usage: python scripts/bench_uvmap.py [--steps 20] [--warmup 5]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import synth, uvmap  # noqa: E402
from texgs.rasterizer import GaussianRasterizationSettings  # noqa: E402
from texgs.uvnet import UVNet  # noqa: E402

PHASES = ["render", "uv_fwd", "inverse_fwd", "chamfer_and_inverse2", "backward"]


def torch_encode(x, table, lv):
    """fp32 twin of tests/hashgrid_ref.py: gathers, autograd backward (scatter-add into the table)."""
    rows = table.reshape(-1, 4)
    outs = []
    for s, res, size, off in zip(lv["scale"], lv["res"], lv["size"], lv["offset"]):
        pos = x * s + 0.5
        fl = torch.floor(pos.detach())
        f = pos - fl
        gi = fl.to(torch.int64) & 0xFFFFFFFF
        hashed = res ** 3 > size
        acc = 0
        for c in range(8):
            cc = (c & 1, (c >> 1) & 1, c >> 2)
            p0, p1, p2 = ((gi[:, d] + cc[d]) & 0xFFFFFFFF for d in range(3))
            if hashed:
                idx = p0 ^ ((p1 * 2654435761) & 0xFFFFFFFF) ^ ((p2 * 805459861) & 0xFFFFFFFF)
            else:
                idx = (p0 + p1 * res + p2 * res * res) & 0xFFFFFFFF
            idx = idx % size
            w = (f[:, 0] if cc[0] else 1 - f[:, 0]) * (f[:, 1] if cc[1] else 1 - f[:, 1]) * (f[:, 2] if cc[2] else 1 - f[:, 2])
            acc = acc + w[:, None] * rows[off + idx]
        outs.append(acc)
    return torch.cat(outs, 1)


def torch_chamfer(x, y):
    d = torch.cdist(x, y) ** 2
    return d.min(dim=1).values.mean() + d.min(dim=0).values.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-gaussians", type=int, default=300_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--pcd", type=int, default=16384)
    ap.add_argument("--only", choices=["hip", "baseline", "both"], default="both")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, W = args.num_gaussians, args.size
    scene = synth.make_scene(N, 4, seed=0)
    cam = synth.fibonacci_cameras(64, W, W)[0]
    st = GaussianRasterizationSettings(image_height=W, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                       bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
                                       projmatrix=cam.full_proj_transform.to(dev), sh_degree=0, campos=cam.camera_center.to(dev),
                                       prefiltered=False, debug=False)
    f = lambda t: t.float().to(dev).contiguous()
    gauss = [f(scene.means3D), f(scene.opacities), f(scene.scales), f(scene.rotations)]
    full_proj = f(cam.full_proj_transform)
    torch.manual_seed(0)
    uv_net = UVNet().to(dev)
    inv_net = uvmap.InvUVNet().to(dev)
    geo_emb = torch.nn.Embedding(1, 128).to(dev)
    pcd = gauss[0][torch.randperm(N, device=dev)[:args.pcd]].contiguous()
    lv = uvmap.hashgrid_levels()
    znear, zfar = 0.01, 100.0

    def iteration(mode, ev):
        ev[0].record()
        depth, alpha = uvmap.render_depth_alpha(st, *gauss)
        ev[1].record()
        emb = geo_emb.weight[0]
        world = uvmap.depth2world(depth[0], full_proj, zfar, znear).reshape(-1, 3)
        wx = world[alpha.reshape(-1) > 0.5].contiguous()
        uv, _ = uv_net.uvs_and_jacobian_with_grad(wx, emb)
        ev[2].record()
        s_uv = inv_net.sample(device=dev)
        if mode == "hip":
            inv = inv_net(uv, emb)
            s_xyz = inv_net(s_uv, emb)
        else:
            inv_f = lambda u: uvmap._InvMLP.apply(torch_encode(u / 2 + 0.5, inv_net.encoding.params, lv), emb, *inv_net._weights())
            inv = inv_f(uv)
            s_xyz = inv_f(s_uv)
        Linv = ((wx - inv) ** 2).sum(-1).mean()
        ev[3].record()
        Lch = uvmap.chamfer_distance(s_xyz[None], pcd[None])[0] if mode == "hip" else torch_chamfer(s_xyz, pcd)
        s_inv_uv, _ = uv_net.uvs_and_jacobian_with_grad(s_xyz, emb)
        Linv2 = ((s_inv_uv - s_uv) ** 2).sum(-1).mean()
        loss = Linv + Lch + Linv2
        ev[4].record()
        loss.backward()
        ev[5].record()
        for p in list(uv_net.parameters()) + list(inv_net.parameters()) + list(geo_emb.parameters()):
            p.grad = None
        return int(wx.shape[0]), float(loss.detach())    # (the float() syncs once per iteration, after the last event)

    out = {"metric": "stage-2 (UV-map) iteration, C3 scene %dx%d, median ms" % (W, W), "unit": "ms/iteration", "num_gaussians": N,
           "pcd_points": args.pcd, "steps": args.steps}
    for mode in (["hip", "baseline"] if args.only == "both" else [args.only]):
        rows = []
        for k in range(args.warmup + args.steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            n_valid, loss = iteration(mode, ev)
            torch.cuda.synchronize()
            if k >= args.warmup:
                rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(5)] + [ev[0].elapsed_time(ev[5])])
        t = torch.tensor(rows)
        med = t.median(dim=0).values.tolist()
        out["valid_points"] = n_valid
        out[mode] = {"ms": round(med[-1], 4), "split_ms": {n: round(v, 4) for n, v in zip(PHASES, med[:5])}, "loss": loss}
    if "hip" in out:
        out["value"] = out["hip"]["ms"]
    if "hip" in out and "baseline" in out:
        out["speedup_vs_baseline"] = round(out["baseline"]["ms"] / out["hip"]["ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
