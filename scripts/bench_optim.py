#!/usr/bin/env python3
"""The optimizer phase of one training iteration -- three Adam steps and the clearing of the gradients, what the reference's
optimize_step does after backward (models/texture_gaussian3d.py:420-444) -- through texgs.optim (csrc/optim.hip) and through torch's
own Adam paths, on the same GPU in the same process.

Parameter set: the C3 texture stage.  N = 300 000 Gaussians (xyz, opacity, scaling, rotation, N x 15 x 3 shs: `optimizer`), the UVNet and
InvUVNet parameter tensors as texgs.uvnet / texgs.uvmap create them (`optimizer_uv`), the 6 x 1024^2 x 3 texture (`optimizer_tex`).

Cases, each one "phase" = three steps + gradients cleared:
  torch_default        torch.optim.Adam (foreach on the device) x 3, zero_grad(set_to_none=False) x 3
  torch_foreach_false  the single-tensor path, likewise
  torch_fused          torch.optim.Adam(fused=True), likewise
  fused_adam_steps     three FusedAdam.step() calls, zero_grad(set_to_none=False) x 3
  fused_adam_steps_zg  three FusedAdam.step(zero_grads=True) calls
  fused_step           one texgs.optim.fused_step([...], zero_grads=True)

Every case owns its tensors (the same values), is warmed up, and the timed phases alternate between the cases; a timing is a pair of
device events around one phase inside a synchronised window, the host clock around the same window is recorded next to it.  The
gradients are refilled outside the window.  Each phase is timed twice: on an idle queue (the window then holds the host's time to
issue the first launch) and `queued_*`, with --queue-copies device copies enqueued ahead of the window, as a backward is in a training
loop, so that the host issues the phase while the device is still busy and the window holds device work only.  Reported: median and minimum over --reps phases (at least 50).

Bytes: one Adam step has to read p, g, m, v and write p, m, v: 28 B per element, 32 B when it also zeroes g.  `GBps` is that over the
phase's device time; `copy` is a plain device-to-device copy moving the same number of bytes (half read, half written): the ceiling.

Writes profiles/optim_bench.json (or --out) and prints one JSON summary line.
Usage: python scripts/bench_optim.py [--reps 50] [--warmup 10] [--n 300000] [--res 1024] [--queue-copies 8] [--out FILE]"""
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

from texgs import optim, uvmap, uvnet  # noqa: E402

EPS = 1e-15
LRS = {"xyz": 1.6e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3, "sh": 1.25e-4}


def make_values(n, res, dev, seed=0):
    """-> [gaussian tensors by name, uv tensors, texture] as plain device tensors, seeded"""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    gauss = {"xyz": rn(n, 3), "opacity": rn(n, 1), "scaling": rn(n, 3), "rotation": rn(n, 4), "sh": rn(n, 15, 3)}
    torch.manual_seed(seed)
    uv = [p.detach().to(dev).clone() for net in (uvnet.UVNet(), uvmap.InvUVNet()) for p in net.parameters() if p.requires_grad]
    tex = rn(6, res, res, 3)
    return gauss, uv, tex


def make_case(values, cls, **kw):
    """Three optimizers of class `cls` over fresh copies of `values`, one step taken, so that the moments exist -> (optimizers, params)"""
    gauss, uv, tex = values
    pg = {k: torch.nn.Parameter(v.clone()) for k, v in gauss.items()}
    pu = [torch.nn.Parameter(v.clone()) for v in uv]
    pt = torch.nn.Parameter(tex.clone())
    opts = [cls([{"params": [p], "lr": LRS[k], "name": k} for k, p in pg.items()], lr=0.0, eps=EPS, **kw),
            cls(pu, lr=2e-5, eps=EPS, **kw),
            cls([pt], lr=2.5e-3, eps=EPS, **kw)]
    params = list(pg.values()) + pu + [pt]
    for p in params:
        p.grad = torch.full_like(p, 1e-3)
    for o in opts:
        o.step()
    return opts, params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=300000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--queue-copies", type=int, default=8, help="device copies enqueued ahead of a `queued` window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs an MI355X: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    values = make_values(a.n, a.res, dev)

    def steps_then_zero_grad(opts):
        def run():
            for o in opts:
                o.step()
            for o in opts:
                o.zero_grad(set_to_none=False)
        return run

    def steps_zeroing(opts):
        def run():
            for o in opts:
                o.step(zero_grads=True)
        return run

    cases = {}
    for name, cls, kw, phase in [
            ("torch_default", torch.optim.Adam, {}, steps_then_zero_grad),
            ("torch_foreach_false", torch.optim.Adam, {"foreach": False}, steps_then_zero_grad),
            ("torch_fused", torch.optim.Adam, {"fused": True}, steps_then_zero_grad),
            ("fused_adam_steps", optim.FusedAdam, {}, steps_then_zero_grad),
            ("fused_adam_steps_zg", optim.FusedAdam, {}, steps_zeroing),
            ("fused_step", optim.FusedAdam, {}, lambda opts: (lambda: optim.fused_step(opts, zero_grads=True)))]:
        opts, params = make_case(values, cls, **kw)
        cases[name] = (phase(opts), params)
    numel = sum(p.numel() for p in cases["fused_step"][1])
    tensors = len(cases["fused_step"][1])
    bytes_step, bytes_step_zero = 28 * numel, 32 * numel
    src = torch.empty(bytes_step_zero // 2, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    cases["copy"] = ((lambda: dst.copy_(src)), [])

    def refill(params):
        for p in params:
            p.grad.fill_(1e-3)

    def timed(run, params, queued=False):
        refill(params)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if queued:              # work ahead of the window, as a backward is in a training loop: the host issues the phase while it runs
            for _ in range(a.queue_copies):
                dst.copy_(src)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    for _ in range(a.warmup):
        for run, params in cases.values():
            timed(run, params)
            timed(run, params, queued=True)
    ev = {k: [] for k in cases}
    evq = {k: [] for k in cases}
    wall = {k: [] for k in cases}
    for _ in range(max(a.reps, 1)):
        for k, (run, params) in cases.items():          # alternate: drift and other people's work hit every case alike
            d, w = timed(run, params)
            ev[k].append(d)
            wall[k].append(w)
            evq[k].append(timed(run, params, queued=True)[0])
    # the cases computed the same thing: every case's parameters after the same number of phases, against the single-tensor path
    agree = {}
    ref = cases["torch_foreach_false"][1]
    for k, (_, params) in cases.items():
        if params:
            agree[k] = max(float((p.detach() - q.detach()).abs().max() / (q.detach().abs().max() + 1e-30)) for p, q in zip(params, ref))

    rows = {}
    for k in cases:
        med, mn = float(np.median(ev[k])), float(np.min(ev[k]))
        medq, mnq = float(np.median(evq[k])), float(np.min(evq[k]))
        nbytes = bytes_step_zero if k in ("fused_adam_steps_zg", "fused_step", "copy") else None
        rows[k] = {"device_ms_median": round(med, 4), "device_ms_min": round(mn, 4), "host_ms_median": round(float(np.median(wall[k])), 4),
                   "queued_device_ms_median": round(medq, 4), "queued_device_ms_min": round(mnq, 4)}
        if nbytes:
            rows[k].update(bytes=nbytes, GBps_median=round(nbytes / med / 1e6, 1), GBps_best=round(nbytes / mn / 1e6, 1),
                           queued_GBps_median=round(nbytes / medq / 1e6, 1), queued_GBps_best=round(nbytes / mnq / 1e6, 1))
        if k in agree:
            rows[k]["max_rel_diff_from_torch_foreach_false"] = agree[k]
    ours = rows["fused_step"]["device_ms_median"]
    for k in ("torch_default", "torch_foreach_false", "torch_fused"):
        rows[k]["ratio_to_fused_step"] = round(rows[k]["device_ms_median"] / ours, 3)
        rows[k]["queued_ratio_to_fused_step"] = round(rows[k]["queued_device_ms_median"] / rows["fused_step"]["queued_device_ms_median"], 3)
    out = {"metric": "one optimizer phase (three Adam steps + gradients cleared), device-event ms, median and minimum over the repetitions",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "warmup": a.warmup, "N": a.n, "tex_res": a.res,
           "tensors": tensors, "elements": numel, "bytes_per_element": {"step": 28, "step_with_zero_grads": 32},
           "bytes_step": bytes_step, "bytes_step_with_zero_grads": bytes_step_zero, "cases": rows,
           "fused_step_share_of_copy": round(rows["copy"]["device_ms_median"] / ours, 3),
           "queued_fused_step_share_of_copy": round(rows["copy"]["queued_device_ms_median"] / rows["fused_step"]["queued_device_ms_median"], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "optim", "elements": numel, **{k: r["device_ms_median"] for k, r in rows.items()},
                      "fused_step_GBps": rows["fused_step"]["GBps_median"], "copy_GBps": rows["copy"]["GBps_median"],
                      "queued": {k: r["queued_device_ms_median"] for k, r in rows.items()}}))


if __name__ == "__main__":
    main()
