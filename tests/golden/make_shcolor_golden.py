"""Generate tests/golden/shcolor.npz: what the reference's own code computes for the colour stage, recorded once.

    python tests/golden/make_shcolor_golden.py --reference /path/to/the/reference/checkout

It imports the reference's utils/sh.py (eval_sh) from that checkout, runs it and the lines of render/render.py:64-68 around it in torch
on the CPU, and stores ARRAYS only -- no program text of the reference ends up in the file or in this repository.  The tests never
need the reference: they read the .npz.

For every degree 0..4, on N = 160 rows with K = 25 standard-normal coefficients per channel, points 2 to 6 units from the camera:
    dirs32_<d>     float32 [N,3]   dir_pp / dir_pp.norm(dim=1, keepdim=True), torch float32 on the CPU
    eval32_<d>     float32 [N,3]   eval_sh(d, shs_view, dirs32) in float32, shs_view the transposed view render.py builds
    colors32_<d>   float32 [N,3]   clamp_min(eval32 + 0.5, 0)
    colors64_<d>   float64 [N,3]   lines 64-68 in float64
    d_sh64_<d>     float64 [N,(d+1)^2,3]   autograd of sum(colors64 * g) to the features (the inactive coefficients' gradient is
                                   asserted to be zero here and not stored)
    d_xyz64_<d>    float64 [N,3]   ... to xyz (zeros at degree 0, where autograd returns None)
    eval64_<d>, d_dirs64_<d>       eval_sh in float64 on float64(dirs32) and autograd of sum(eval64 * g) to the directions
and the constructed degree-0 rows: float32 coefficients s around -0.5 / C0 with torch's float32 clamp_min(C0 * s + 0.5, 0) and its
gradient to s (upstream one) -- among them those whose C0 * s + 0.5 is EXACTLY zero in float32, where clamp_min passes the gradient."""
import argparse
import importlib.util
import os

import numpy as np
import torch

N, K = 160, 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (utils/sh.py is imported from it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "shcolor.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_sh", os.path.join(a.reference, "utils", "sh.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(20261021)
    features = rng.standard_normal((N, K, 3)).astype(np.float32)
    u = rng.standard_normal((N, 3))
    campos = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
    xyz = (campos + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (N, 1))).astype(np.float32)
    g = rng.standard_normal((N, 3)).astype(np.float32)
    out = dict(features=features, xyz=xyz, campos=campos, g=g)

    def glue(feat, pts, cam, deg):
        """the composition of render.py:64-68 around the reference's eval_sh: transposed coefficient view, offset from the camera
        centre over its norm, eval_sh, + 0.5, clamp at zero"""
        coeffs_cf = feat.transpose(1, 2).view(-1, 3, K)
        offset = pts - cam.repeat(feat.shape[0], 1)
        unit = offset / offset.norm(dim=1, keepdim=True)
        raw = ref.eval_sh(deg, coeffs_cf, unit)
        return torch.clamp_min(raw + 0.5, 0.0), raw, unit

    for deg in range(5):
        f32, p32, c32 = torch.tensor(features), torch.tensor(xyz), torch.tensor(campos).reshape(1, 3)
        col, ev, dirs = glue(f32, p32, c32, deg)
        assert col.dtype == torch.float32
        out[f"dirs32_{deg}"], out[f"eval32_{deg}"], out[f"colors32_{deg}"] = dirs.numpy(), ev.numpy(), col.numpy()
        f64 = torch.tensor(features, dtype=torch.float64, requires_grad=True)
        p64 = torch.tensor(xyz, dtype=torch.float64, requires_grad=True)
        col64, _, _ = glue(f64, p64, c32.double(), deg)
        (col64 * torch.tensor(g, dtype=torch.float64)).sum().backward()
        A = (deg + 1) ** 2
        assert not f64.grad[:, A:, :].any()
        out[f"colors64_{deg}"] = col64.detach().numpy()
        out[f"d_sh64_{deg}"] = f64.grad[:, :A, :].numpy().copy()
        out[f"d_xyz64_{deg}"] = np.zeros((N, 3)) if p64.grad is None else p64.grad.numpy()
        d64 = dirs.double().clone().requires_grad_(True)
        e64 = torch.tensor(features, dtype=torch.float64, requires_grad=True)      # (so that degree 0, which has no direction, has a graph)
        ev64 = ref.eval_sh(deg, e64.transpose(1, 2).view(-1, 3, K), d64)
        (ev64 * torch.tensor(g, dtype=torch.float64)).sum().backward()
        out[f"eval64_{deg}"] = ev64.detach().numpy()
        out[f"d_dirs64_{deg}"] = np.zeros((N, 3)) if d64.grad is None else d64.grad.numpy()
        clamped = float((col == 0).float().mean())
        print(f"degree {deg}: {100 * clamped:.1f} % of the entries clamped")

    # degree 0 at the clamp's edge: the floats around -0.5 / C0
    c0 = np.float32(ref.C0)
    s0 = np.float32(-0.5) / c0
    cand = [s0]
    lo = hi = s0
    for _ in range(24):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        cand += [lo, hi]
    cand = np.sort(np.array(cand, np.float32))
    s = torch.tensor(cand, requires_grad=True)
    sh = s.reshape(-1, 1, 1).expand(-1, 3, 1)
    col = torch.clamp_min(ref.eval_sh(0, sh, torch.zeros(cand.size, 3)) + 0.5, 0.0)
    col[:, 0].sum().backward()
    exact = (c0 * cand + np.float32(0.5)) == 0
    print(f"edge rows: {cand.size} candidates, {int(exact.sum())} with C0 * s + 0.5 exactly zero; gradient there:", s.grad.numpy()[exact])
    out["edge_sh"], out["edge_color"], out["edge_grad"], out["edge_exact"] = cand, col[:, 0].detach().numpy(), s.grad.numpy(), exact
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
