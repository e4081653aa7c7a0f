#!/usr/bin/env python3
"""LPIPS-VGG of one pair as a LOSS -- forward and backward, img0 differentiable -- two ways, timed in the same process, at 800x800 and
1600x1200, random weights (LPIPSVGG.random):

  torch   the composition the lpips package executes, as torch ops on the device under autograd: the scaling layer, F.conv2d + relu +
          max_pool2d through the thirteen convolutions, per tapped layer normalise / subtract / square / 1x1 weights / spatial mean,
          then .backward()
  fp32    texgs.lpips.LPIPSVGG: the forward's thirteen k_conv3x3 and five heads with every map kept, then the backward of
          texgs/lpips_grad.py -- five k_lpips_head_backward, thirteen k_conv3x3 over transposed weights (P images: one side is
          differentiable), eight k_lpips_gate and one multiply

Every leg is host wall clock around a call that ends synchronised, legs alternating inside one loop; medians and p10-p90 of --reps
after --warmup.  verdict: "faster" / "slower" when the medians differ by more than the torch leg's own p10-p90 spread, "tie" inside it
(the rule of scripts/bench_lpips.py).  No pass mark is set on these numbers.  peak_extra_mb is torch.cuda.max_memory_allocated over
one call minus what was allocated before it.

--trace-legs N runs N forward + backward calls of the fp32 leg per size and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --`; --reduce-trace FILE turns that run's kernel trace (a CSV with Kernel_Name, Start_Timestamp,
End_Timestamp per dispatch) into profiles/lpips_grad_kernel_stats.csv: per size the median time per call of the forward's
convolutions, the data-gradient convolutions, conv1_1's gradient among them (a 64-channel tile computed for 3 channels), the head's
backward, the gates, and the streaming kernels' share of the backward.

Writes profiles/lpips_grad_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_lpips_grad.py [--reps 30] [--warmup 5] [--out FILE]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(800, 800), (1600, 1200)]
SLICES = (2, 2, 3, 3, 3)


def torch_leg(net, device):
    import torch
    import torch.nn.functional as F
    convs = [(w.to(device), b.to(device)) for w, b in net.convs]
    lins = [l.to(device).view(1, -1, 1, 1) for l in net.lins]
    shift = torch.tensor([-0.030, -0.088, -0.188], device=device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=device).view(1, 3, 1, 1)

    def run(a, b):
        a.grad = None
        x = (2 * torch.stack([a, b]) - 1 - shift) / scale
        total, k = 0, 0
        for s, n in enumerate(SLICES):
            if s > 0:
                x = F.max_pool2d(x, 2)
            for _ in range(n):
                x = F.conv2d(x, convs[k][0], convs[k][1], padding=1).relu()
                k += 1
            f = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            total = total + (lins[s] * (f[:1] - f[1:]) ** 2).sum(dim=1, keepdim=True).mean([2, 3], keepdim=True)
        total.sum().backward()
        return total.detach(), a.grad
    return run


def ours_leg(net):
    def run(a, b):
        a.grad = None
        v = net(a, b, normalize=True)
        v.sum().backward()
        return v.detach(), a.grad
    return run


def wall_ms(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def reduce_trace(path, out, calls):
    """Kernel trace of a --trace-legs run -> per size the median time per call of each group of kernels.  Per call and in time order
    the 26 convolution dispatches are the forward's thirteen, then the thirteen data gradients, conv1_1's last."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    pick = lambda word, skip=None: [r for r in rows if word in r["Kernel_Name"] and not (skip and skip in r["Kernel_Name"])]
    conv, hb, gate, hf = pick("k_conv3x3", "pack"), pick("k_lpips_head_backward"), pick("k_lpips_gate"), pick("k_lpips_head", "backward")
    want = {"k_conv3x3": (conv, 26), "k_lpips_head_backward": (hb, 5), "k_lpips_gate": (gate, 8), "k_lpips_head": (hf, 10)}
    for name, (lst, per) in want.items():
        if len(lst) != per * calls * len(SIZES):
            raise SystemExit(f"{len(lst)} dispatches of {name} in {path}, expected {per * calls * len(SIZES)}")
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["size", "group", "dispatches_per_call", "median_us_per_call", "share_of_backward"])
        for si, (H, W) in enumerate(SIZES):
            part = lambda lst, per: [lst[(si * calls + c) * per:(si * calls + c + 1) * per] for c in range(calls)]
            med = lambda groups: float(np.median([sum(us(r) for r in g) for g in groups]))
            cv = part(conv, 26)
            t = {"forward k_conv3x3": (13, med([g[:13] for g in cv])), "forward k_lpips_head + reduce": (10, med(part(hf, 10))),
                 "backward k_conv3x3 (data gradients)": (13, med([g[13:] for g in cv])),
                 "backward k_conv3x3, conv1_1's gradient alone": (1, med([g[25:] for g in cv])),
                 "backward k_lpips_head_backward": (5, med(part(hb, 5))), "backward k_lpips_gate": (8, med(part(gate, 8)))}
            bwd = t["backward k_conv3x3 (data gradients)"][1] + t["backward k_lpips_head_backward"][1] + t["backward k_lpips_gate"][1]
            for name, (n, v) in t.items():
                wr.writerow([f"{H}x{W}", name, n, round(v, 1), round(v / bwd, 4) if name.startswith("backward") else ""])
            stream = t["backward k_lpips_head_backward"][1] + t["backward k_lpips_gate"][1]
            wr.writerow([f"{H}x{W}", "backward streaming kernels (head backward + gates)", 13, round(stream, 1), round(stream / bwd, 4)])
            wr.writerow([f"{H}x{W}", "backward, these three kernels", 26, round(bwd, 1), 1.0])
    print(json.dumps({"reduced": out, "dispatches": len(conv) + len(hb) + len(gate) + len(hf)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_grad_bench.json"))
    ap.add_argument("--trace-legs", type=int, default=0)
    ap.add_argument("--reduce-trace", default=None)
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "lpips_grad_kernel_stats.csv"))
    a = ap.parse_args()
    if a.reduce_trace:
        return reduce_trace(a.reduce_trace, a.stats_out, a.trace_calls)
    import torch
    from texgs import lpips
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_grad.py needs an MI355X")
    dev = torch.device("cuda")
    net = lpips.LPIPSVGG.random(1)
    gen = torch.Generator().manual_seed(2)
    ours = ours_leg(net)
    if a.trace_legs:
        for H, W in SIZES:
            x, y = (torch.rand(3, H, W, generator=gen).to(dev) for _ in range(2))
            x.requires_grad_()
            for _ in range(a.trace_legs):
                ours(x, y)
            torch.cuda.synchronize()
        return
    ref = torch_leg(net, dev)
    rows = []
    for H, W in SIZES:
        x, y = (torch.rand(3, H, W, generator=gen).to(dev) for _ in range(2))
        x.requires_grad_()
        legs = {"torch": lambda: ref(x, y), "fp32": lambda: ours(x, y)}
        first, peak = {}, {}
        for k, f in legs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            v, g = f()
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - before) / 1e6
            first[k] = (float(v.reshape(-1)[0].item()), g.detach().clone())
            x.grad = None
        gdiff = float((first["torch"][1] - first["fp32"][1]).abs().max())
        gmax = float(first["torch"][1].abs().max())
        for _ in range(a.warmup):
            for f in legs.values():
                f()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                ms[k].append(wall_ms(f))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        p = {k: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for k, v in ms.items()}
        spread = p["torch"][1] - p["torch"][0]
        diff = med["torch"] - med["fp32"]
        rows.append({"H": H, "W": W, "pairs": 1, "differentiable": "img0",
                     "torch_ms": round(med["torch"], 3), "torch_p10_p90_ms": [round(v, 3) for v in p["torch"]],
                     "fp32_ms": round(med["fp32"], 3), "fp32_p10_p90_ms": [round(v, 3) for v in p["fp32"]],
                     "torch_p10_p90_spread_ms": round(spread, 3), "torch_over_fp32": round(med["torch"] / med["fp32"], 3),
                     "verdict": "tie" if abs(diff) <= spread else ("faster" if diff > 0 else "slower"),
                     "peak_extra_mb": {k: round(v, 1) for k, v in peak.items()},
                     "kept_activation_mb": round(lpips.grad_activation_floats(1, H, W) * 4 / 1e6, 1),
                     "lpips": {k: v[0] for k, v in first.items()},
                     "grad_max_abs": gmax, "grad_max_abs_difference_between_the_legs": gdiff})
    out = {"metric": "host wall-clock ms of one LPIPS-VGG pair as a loss: forward + backward with img0 differentiable, a call that ends "
                     "synchronised; medians and p10-p90 of alternating repetitions in one process; verdict of the fp32 leg against the torch "
                     "leg's own p10-p90 spread; no pass mark; peak_extra_mb: peak allocation over one call above what was allocated before it",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "warmup": a.warmup, "weights": "LPIPSVGG.random(1)",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "lpips_grad", **{f"{r['H']}x{r['W']}": {k: r[k] for k in ("torch_ms", "fp32_ms", "verdict")} for r in rows}}))


if __name__ == "__main__":
    main()
