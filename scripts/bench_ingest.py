#!/usr/bin/env python3
"""The input stage two ways, timed in the same process: the reference's own lines (Pillow's resize on one core, a host division, a
permute, a float32 upload, the mask product on the device) against texgs.ingest (the bytes uploaded, everything else in HIP).

  camera     one view with rgb, alpha and normal, from host uint8 images to the three device tensors of `Camera`, at
             1600x1200 -> 800x600 and at 800x800 unchanged: utils/general.py:21-27 + utils/cameras.py:103-122, 44-54 against
             `camera_images` on host arrays (its pageable upload included)
  resident   the same `camera_images` on bytes that are already on the device: device-event time per call with --batch calls
             between one event pair, and the algorithmic bytes (read once, written once, from the shapes) over it.  Twelve launches
             with a resize (two tap tables and two passes per image), three without: at these sizes that is enqueue as much as
             kernel, so call_gbps is a floor for the kernels' rate
  uploader   --cameras views through `ViewUploader(4)`, submit to drained and synchronised, as views per second

Every leg is host wall clock around a call that ends synchronised, the two legs alternating inside one loop; medians with p10-p90.
verdict: "faster" / "slower" when the medians differ by more than the wider of the two spreads, "tie" inside it.  The results of the
two legs are compared in this run (max_difference_from_reference); the bit-exact comparison is the test suite's.
Without Pillow the reference leg is left out ("pillow": "absent").

Writes profiles/ingest_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_ingest.py [--reps 30] [--batch 20] [--warmup 2] [--cameras 64] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "texture-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from texgs import ingest  # noqa: E402

try:
    from PIL import Image
    import PIL
except ImportError:
    Image = None


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def batch_ms(f, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(k):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "p10_p90_ms": [round(float(np.percentile(v, q)), 3) for q in (10, 90)]}


# ---- the reference's lines ----
def pil_to_torch(pil_image, resolution):                   # utils/general.py:21-27
    resized = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return resized.permute(2, 0, 1) if len(resized.shape) == 3 else resized.unsqueeze(dim=-1).permute(2, 0, 1)


def ref_camera(image, alpha, normal, resolution):          # utils/cameras.py:103-122 and Camera.__init__ :44-54
    rgb, a, n = pil_to_torch(image, resolution), pil_to_torch(alpha, resolution), pil_to_torch(normal, resolution)
    mask = (a[0:1, ...] > 0).float()
    gt_normal = n[:3, ...] * 2. - 1.
    original = rgb[:3, ...].clamp(0.0, 1.0).to("cuda")
    original *= mask.to("cuda")
    return original, mask.to("cuda"), gt_normal.to("cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="alternating timed repetitions per row")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs an MI355X: there is no CPU path to time")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for (H, W), res in (((1200, 1600), (800, 600)), ((800, 800), (800, 800))):
        rng = np.random.default_rng(H + W)
        image, normal = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
        alpha = np.repeat((rng.integers(0, 4, (H, W, 1)) > 0).astype(np.uint8) * 255, 3, axis=2)
        shape = {"source": [H, W], "resolution": list(res)}
        ours = lambda: ingest.camera_images(image, res, alpha=alpha, normal=normal)        # noqa: E731
        row = {"row": "camera", **shape, "upload_mb": {"reference": round(8 * res[0] * res[1] * 4 / 1e6, 2), "ingest": round(3 * H * W * 3 / 1e6, 2)}}
        if Image is None:
            for _ in range(args.warmup):
                ours()
            row.update({"pillow": "absent", "ingest": stats([wall_ms(ours) for _ in range(args.reps)])})
        else:
            pil = [Image.fromarray(x) for x in (image, alpha, normal)]
            ref = lambda: ref_camera(*pil, res)            # noqa: E731
            row["max_difference_from_reference"] = max(float((a - b).abs().max()) for a, b in zip(ref(), ours()))
            for _ in range(args.warmup):
                ref(), ours()
            t_ref, t_ours = [], []
            for _ in range(args.reps):
                t_ref.append(wall_ms(ref))
                t_ours.append(wall_ms(ours))
            r, o = stats(t_ref), stats(t_ours)
            spread = max(s["p10_p90_ms"][1] - s["p10_p90_ms"][0] for s in (r, o))
            d = r["median_ms"] - o["median_ms"]
            row.update({"reference": r, "ingest": o, "reference_over_ingest": round(r["median_ms"] / o["median_ms"], 2),
                        "verdict": "tie" if abs(d) <= spread else ("faster" if d > 0 else "slower")})
        emit(row)
        # the kernels alone: the same call on bytes that are already on the device, --batch calls between one pair of events
        on_dev = [torch.from_numpy(x).cuda() for x in (image, alpha, normal)]
        resident = lambda: ingest.camera_images(on_dev[0], res, alpha=on_dev[1], normal=on_dev[2])        # noqa: E731
        resident()
        t = [batch_ms(resident, args.batch) for _ in range(5)]
        nbytes = 3 * H * W * 3 + res[0] * res[1] * 4 * (3 + 1 + 1 + 3)          # three sources read; mask written and read, two images written
        emit({"row": "resident", **shape, "launches": 12 if (W, H) != tuple(res) else 3, "batch": args.batch,
              "call_batched_ms": round(float(np.median(t)), 4), "algorithmic_mb": round(nbytes / 1e6, 2),
              "call_gbps": round(nbytes / (float(np.median(t)) * 1e-3) / 1e9, 1)})
        del on_dev
        # the uploader
        up = ingest.ViewUploader(4, H, W)

        def loop():
            for k in range(args.cameras):
                up.submit(k, image, res, alpha=alpha, normal=normal)
            return [outs for _, outs in up.drain()]
        loop()
        t = [wall_ms(loop) for _ in range(max(3, args.reps // 3))]
        s = stats(t)
        emit({"row": "uploader", **shape, "cameras": args.cameras, "ring": 4, **s,
              "views_per_second": round(args.cameras / (s["median_ms"] * 1e-3), 1),
              "ms_per_view": round(s["median_ms"] / args.cameras, 3)})
        del up
        torch.cuda.empty_cache()

    out = {"metric": "host wall-clock ms of a call that ends synchronised; medians and p10-p90 of alternating repetitions in one process; "
                     "verdict against the wider of the two legs' p10-p90 spreads",
           "device": torch.cuda.get_device_name(0), "pillow": "absent" if Image is None else PIL.__version__,
           "host_threads": torch.get_num_threads(), "reps": args.reps, "warmup": args.warmup,
           "slower_rows": [{"row": r["row"], "source": r["source"]} for r in rows if r.get("verdict") == "slower"],
           "tied_rows": [{"row": r["row"], "source": r["source"]} for r in rows if r.get("verdict") == "tie"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)


if __name__ == "__main__":
    main()
