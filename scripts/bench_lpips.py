#!/usr/bin/env python3
"""LPIPS-VGG of one pair two ways, timed in the same process, at 800x800 and 1600x1200, random weights (LPIPSVGG.random):

  torch   the composition the lpips package executes, as torch ops on the device: the scaling layer, F.conv2d + relu_ + max_pool2d
          through the thirteen convolutions, and per tapped layer normalise / subtract / square / 1x1 weights / spatial mean
  fp32    texgs.lpips.LPIPSVGG(precision="fp32"): thirteen launches of k_conv3x3 and five heads (csrc/lpips.hip)
("bf16x3" is not built, so it has no leg.)

Every leg is host wall clock around a call that ends synchronised, legs alternating inside one loop; medians and p10-p90 of --reps
after --warmup.  verdict: "faster" / "slower" when the medians differ by more than the torch leg's own p10-p90 spread, "tie" inside it
(the rule of scripts/bench_present.py).  tflops = the layer table's FLOPs (2 x 9 Cin Cout Ho Wo per image and convolution, both
images) over the median.

--trace-legs N runs N calls of the fp32 leg per size and nothing else: the program to put behind `rocprofv3 --kernel-trace --stats --`;
--reduce-trace FILE turns that run's kernel trace (a CSV with Kernel_Name, Start_Timestamp, End_Timestamp per dispatch) into
profiles/lpips_kernel_stats.csv: per size and layer the median kernel time and its TFLOP/s.

Writes profiles/lpips_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_lpips.py [--reps 30] [--warmup 5] [--out FILE]"""
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
WIDTHS = (64, 128, 256, 512, 512)
NAMES = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2",
         "conv5_3"]


def layer_table(H, W, images=2):
    """[(name, Cin, Cout, Ho, Wo, FLOPs over `images` images)] of the thirteen convolutions"""
    rows, cin, h, w, k = [], 3, H, W, 0
    for s, n in enumerate(SLICES):
        for j in range(n):
            if s > 0 and j == 0:
                h, w = h // 2, w // 2
            rows.append((NAMES[k], cin, WIDTHS[s], h, w, 2 * 9 * cin * WIDTHS[s] * h * w * images))
            cin, k = WIDTHS[s], k + 1
    return rows


def torch_leg(net, device):
    import torch
    import torch.nn.functional as F
    convs = [(w.to(device), b.to(device)) for w, b in net.convs]
    lins = [l.to(device).view(1, -1, 1, 1) for l in net.lins]
    shift = torch.tensor([-0.030, -0.088, -0.188], device=device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=device).view(1, 3, 1, 1)

    def run(a, b):
        x = (2 * torch.stack([a, b]) - 1 - shift) / scale
        total, k = 0, 0
        for s, n in enumerate(SLICES):
            if s > 0:
                x = F.max_pool2d(x, 2)
            for _ in range(n):
                x = F.conv2d(x, convs[k][0], convs[k][1], padding=1).relu_()
                k += 1
            f = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            total = total + (lins[s] * (f[:1] - f[1:]) ** 2).sum(dim=1, keepdim=True).mean([2, 3], keepdim=True)
        return total
    return run


def wall_ms(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def reduce_trace(path, out, calls):
    """Kernel trace of a --trace-legs run -> per (size, layer) median kernel time; `calls` fp32 calls per size, sizes in SIZES order"""
    rows = list(csv.DictReader(open(path)))
    conv = [r for r in rows if "k_conv3x3" in r["Kernel_Name"] and "pack" not in r["Kernel_Name"]]
    conv.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(conv) != 13 * calls * len(SIZES):
        raise SystemExit(f"{len(conv)} convolution dispatches in {path}, expected {13 * calls * len(SIZES)}")
    heads = sorted((r for r in rows if "k_lpips_head" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    with open(out, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["size", "kernel", "layer", "Cin", "Cout", "Ho", "Wo", "gflop", "median_us", "min_us", "tflops_at_median"])
        for si, (H, W) in enumerate(SIZES):
            mine = conv[si * 13 * calls:(si + 1) * 13 * calls]
            total = 0.0
            for k, (name, cin, cout, h, w, flops) in enumerate(layer_table(H, W)):
                t = [us(mine[c * 13 + k]) for c in range(calls)]
                med = float(np.median(t))
                total += med
                wr.writerow([f"{H}x{W}", "k_conv3x3", name, cin, cout, h, w, round(flops / 1e9, 3), round(med, 1), round(min(t), 1),
                             round(flops / (med * 1e-6) / 1e12, 2)])
            hs = heads[si * 10 * calls:(si + 1) * 10 * calls]
            head_us = float(np.median([sum(us(r) for r in hs[c * 10:(c + 1) * 10]) for c in range(calls)])) if len(hs) == 10 * calls else float("nan")
            flops = sum(r[5] for r in layer_table(H, W))
            wr.writerow([f"{H}x{W}", "k_lpips_head + reduce", "five layers", "", "", "", "", "", round(head_us, 1), "", ""])
            wr.writerow([f"{H}x{W}", "k_conv3x3", "all thirteen", "", "", "", "", round(flops / 1e9, 3), round(total, 1), "",
                         round(flops / (total * 1e-6) / 1e12, 2)])
    print(json.dumps({"reduced": out, "dispatches": len(conv)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    ap.add_argument("--trace-legs", type=int, default=0)
    ap.add_argument("--reduce-trace", default=None)
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "lpips_kernel_stats.csv"))
    a = ap.parse_args()
    if a.reduce_trace:
        return reduce_trace(a.reduce_trace, a.stats_out, a.trace_calls)
    import torch
    from texgs import lpips
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py needs an MI355X")
    dev = torch.device("cuda")
    net = lpips.LPIPSVGG.random(1)
    gen = torch.Generator().manual_seed(2)
    if a.trace_legs:
        for H, W in SIZES:
            x, y = (torch.rand(3, H, W, generator=gen).to(dev) for _ in range(2))
            for _ in range(a.trace_legs):
                net(x, y, normalize=True)
            torch.cuda.synchronize()
        return
    ref = torch_leg(net, dev)
    rows = []
    for H, W in SIZES:
        x, y = (torch.rand(3, H, W, generator=gen).to(dev) for _ in range(2))
        legs = {"torch": lambda: ref(x, y), "fp32": lambda: net(x, y, normalize=True)}
        values = {k: float(f().reshape(-1)[0].item()) for k, f in legs.items()}
        for _ in range(a.warmup):
            for f in legs.values():
                f()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                ms[k].append(wall_ms(f))
        flops = sum(r[5] for r in layer_table(H, W))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        p = {k: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for k, v in ms.items()}
        spread = p["torch"][1] - p["torch"][0]
        diff = med["torch"] - med["fp32"]
        rows.append({"H": H, "W": W, "pairs": 1, "conv_tflop": round(flops / 1e12, 4),
                     "torch_ms": round(med["torch"], 3), "torch_p10_p90_ms": [round(v, 3) for v in p["torch"]],
                     "fp32_ms": round(med["fp32"], 3), "fp32_p10_p90_ms": [round(v, 3) for v in p["fp32"]],
                     "torch_p10_p90_spread_ms": round(spread, 3), "torch_over_fp32": round(med["torch"] / med["fp32"], 3),
                     "verdict": "tie" if abs(diff) <= spread else ("faster" if diff > 0 else "slower"),
                     "torch_tflops": round(flops / (med["torch"] * 1e-3) / 1e12, 1), "fp32_tflops": round(flops / (med["fp32"] * 1e-3) / 1e12, 1),
                     "lpips": values, "value_difference": abs(values["torch"] - values["fp32"])})
    out = {"metric": "host wall-clock ms of one LPIPS-VGG pair, a call that ends synchronised; medians and p10-p90 of alternating repetitions in "
                     "one process; verdict of the fp32 leg against the torch leg's own p10-p90 spread; tflops = convolution FLOPs of the layer "
                     "table over the median (the f32 matrix peak of the part is 157 TF)",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "warmup": a.warmup, "weights": "LPIPSVGG.random(1)",
           "bf16x3": "not built: no leg", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "lpips", **{f"{r['H']}x{r['W']}": {k: r[k] for k in ("torch_ms", "fp32_ms", "verdict", "fp32_tflops")} for r in rows}}))


if __name__ == "__main__":
    main()
