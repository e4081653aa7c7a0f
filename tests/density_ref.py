"""numpy fp32 statement of texgs.density (csrc/density.hip): the per-step statistics, the plan of a densify_and_prune (action bytes,
exclusive ranks, totals) and the move.  Every operation is rounded to fp32 on its own (`x*x + y*y` with separate roundings, no FMA),
division and sqrt are numpy's correctly rounded ones.  tests/test_density_host.py pins this file to the reference's own functions
through tests/golden/density.npz; the GPU tests compare the kernels with this file."""
import os

import numpy as np

F32 = np.float32
TOL_CHILD = 2e-6        # children's xyz and scaling against the golden, absolute (tests/test_density_host.py explains)
TOL_NORM = 1e-6         # accumulated norms against the golden, relative
KEEP, CLONE, CLONE_KEPT, SPLIT, CHILD = 1, 2, 4, 8, 16
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def stats_np(accum, denom, max_radii, grad, radii):
    """-> (accum [N,1], denom [N,1], max_radii [N]) after one add_densification_stats; inputs untouched"""
    accum, denom, max_radii = accum.astype(F32).copy(), denom.astype(F32).copy(), max_radii.astype(F32).copy()
    vis = radii > 0
    gx, gy = grad[:, 0].astype(F32), grad[:, 1].astype(F32)
    norm = np.sqrt(gx * gx + gy * gy, dtype=F32)
    accum[vis, 0] = accum[vis, 0] + norm[vis]
    denom[vis, 0] = denom[vis, 0] + F32(1)
    max_radii[vis] = np.maximum(max_radii[vis], radii[vis].astype(F32))
    return accum, denom, max_radii


def activations(scaling, opacity):
    """(s f32[N,3], m f32[N], o f32[N]) as the kernels spell them"""
    s = np.exp(scaling.astype(F32), dtype=F32)
    x = opacity.reshape(-1).astype(F32)
    o = F32(1) / (F32(1) + np.exp(-x, dtype=F32))
    return s, s.max(axis=1), o


def child_scaling(s):
    return np.log(s / F32(1.6), dtype=F32)


def plan_np(accum, denom, scaling, opacity, max_grad, min_opacity, dense_scale, big_scale, densify=True, use_big=True):
    """-> (action u8[N], rank i32[4,N] exclusive counts of KEEP / CLONE_KEPT / SPLIT / CHILD, totals i64[4])"""
    n = scaling.shape[0]
    s, m, o = activations(scaling, opacity)
    max_grad, min_opacity, dense_scale, big_scale = F32(max_grad), F32(min_opacity), F32(dense_scale), F32(big_scale)
    low = o < min_opacity
    clone = np.zeros(n, bool)
    split = np.zeros(n, bool)
    if densify:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = accum.reshape(-1).astype(F32) / denom.reshape(-1).astype(F32)
        g = np.where(np.isnan(g), F32(0), g).astype(F32)
        small = m <= dense_scale
        clone = (np.sqrt(g * g, dtype=F32) >= max_grad) & small
        split = (g >= max_grad) & ~small
    mc = np.exp(child_scaling(s), dtype=F32).max(axis=1) if n else m
    child = split & ~(low | (bool(use_big) & (mc > big_scale)))
    keep = ~split & ~(low | (bool(use_big) & (m > big_scale)))
    clone = clone & ~split
    clone_kept = clone & keep
    action = (keep * KEEP + clone * CLONE + clone_kept * CLONE_KEPT + split * SPLIT + child * CHILD).astype(np.uint8)
    flags = np.stack([keep, clone_kept, split, child]).astype(np.int64)
    inc = np.cumsum(flags, axis=1)
    rank = (inc - flags).astype(np.int32)
    totals = inc[:, -1] if n else np.zeros(4, np.int64)
    return action, rank, totals


def build_rotation_np(q):
    """utils/general.py:87-108 in fp32"""
    q = q.astype(F32)
    norm = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3], dtype=F32)
    q = q / norm[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.zeros((q.shape[0], 3, 3), F32)
    one, two = F32(1), F32(2)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (y * z + r * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def move_np(params, moments, action, rank, totals, noise):
    """params {name: f32[N, ...]}, moments {name: (exp_avg, exp_avg_sq) or None} -> (new params, new moments): the surviving originals,
    the surviving clones, the surviving first children, the surviving second children."""
    kept = np.flatnonzero(action & KEEP)
    cl = np.flatnonzero(action & CLONE_KEPT)
    ch = np.flatnonzero(action & CHILD)
    n_split = int(totals[2])
    assert (len(kept), len(cl), len(ch)) == (int(totals[0]), int(totals[1]), int(totals[3]))
    assert np.array_equal(rank[0][kept], np.arange(len(kept))) and np.array_equal(rank[1][cl], np.arange(len(cl)))
    assert np.array_equal(rank[3][ch], np.arange(len(ch)))
    out, out_m = {}, {}
    for name in GROUPS:
        src = params[name].astype(F32)
        c0 = c1 = src[ch]
        if name == "scaling":
            c0 = c1 = child_scaling(np.exp(src[ch], dtype=F32))
        elif name == "xyz" and len(ch):
            s = np.exp(params["scaling"][ch].astype(F32), dtype=F32)
            R = build_rotation_np(params["rotation"][ch])
            j = rank[2][ch]
            both = []
            for c in (0, 1):
                v = s * noise[c * n_split + j].astype(F32)
                rot = (R[:, :, 0] * v[:, None, 0] + R[:, :, 1] * v[:, None, 1]) + R[:, :, 2] * v[:, None, 2]
                both.append((rot + src[ch]).astype(F32))
            c0, c1 = both
        out[name] = np.concatenate([src[kept], src[cl], c0, c1], axis=0)
        if moments.get(name) is None:
            out_m[name] = None
        else:
            new = len(cl) + 2 * len(ch)
            out_m[name] = tuple(np.concatenate([mo.astype(F32)[kept], np.zeros((new,) + mo.shape[1:], F32)], axis=0) for mo in moments[name])
    return out, out_m


def reset_opacity_np(opacity):
    o = F32(1) / (F32(1) + np.exp(-opacity.astype(F32), dtype=F32))
    x = np.minimum(o, F32(0.01))
    return np.log(x / (F32(1) - x), dtype=F32)


def reset_min_scale_np(scaling):
    out = scaling.astype(F32).copy()
    out[np.arange(out.shape[0]), np.argmin(out, axis=1)] = F32(-20.0)
    return out


def cloud(n, seed, width_rest=45, frac=(0.05, 0.05, 0.03), margin=1e-4, max_grad=0.0002, min_opacity=0.005, dense_scale=0.01, big_scale=0.1):
    """A seeded test cloud (numpy): parameters by name, accum / denom, noise for every possible split -- with every compared quantity
    at least `margin` (relative) away from its threshold, so that a last-bit difference between two expf implementations cannot
    change a decision.  frac = (clone, split, prune) shares, roughly."""
    rng = np.random.RandomState(seed)
    u = rng.rand(n)
    scaling = (np.log(0.004) + 0.25 * rng.randn(n, 3)).astype(F32)            # small: m well below dense_scale
    big = u < frac[1] + frac[2] / 2                                            # candidates to split / to prune by size
    scaling[big] = (np.log(0.03) + 0.3 * rng.randn(int(big.sum()), 3)).astype(F32)
    huge = rng.rand(n) < frac[2] / 2
    scaling[huge] = (np.log(0.3) + 0.2 * rng.randn(int(huge.sum()), 3)).astype(F32)
    opacity = (2.0 * rng.randn(n, 1)).astype(F32)
    lowop = rng.rand(n) < frac[2] / 2
    opacity[lowop] = (-7.0 + 0.3 * rng.randn(int(lowop.sum()), 1)).astype(F32)
    denom = rng.randint(0, 6, size=(n, 1)).astype(F32)
    hot = (rng.rand(n) < frac[0] + frac[1] * 3) | big
    g = np.where(hot, max_grad * (1.5 + rng.rand(n)), max_grad * 0.6 * rng.rand(n)).astype(F32)
    accum = (g[:, None] * denom).astype(F32)
    # margins: move whatever sits within `margin` of a threshold clearly to one side
    s, m, o = (a.astype(np.float64) for a in activations(scaling, opacity))
    for thr in (dense_scale, big_scale, big_scale * 1.6):
        near = np.abs(m / thr - 1.0) < 10 * margin
        scaling[near] -= F32(0.01)
    near = np.abs(o / min_opacity - 1.0) < 10 * margin
    opacity[near] -= F32(0.01)
    with np.errstate(divide="ignore", invalid="ignore"):
        gg = (accum / denom).astype(np.float64).reshape(-1)
    near = np.abs(gg / max_grad - 1.0) < 10 * margin
    accum[near] *= F32(1.01)
    params = {"xyz": (4.0 * rng.rand(n, 3) - 2.0).astype(F32), "f_dc": rng.randn(n, 1, 3).astype(F32),
              "f_rest": rng.randn(n, width_rest // 3, 3).astype(F32), "opacity": opacity, "scaling": scaling,
              "rotation": rng.randn(n, 4).astype(F32)}
    noise = rng.randn(2 * n, 3).astype(F32)
    return params, accum, denom, noise


# ---- tests/golden/density.npz (the reference's own results, tests/golden/make_density_golden.py) ----
_GOLD = []


def golden():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density.npz")))
    return _GOLD[0]


def golden_case(tag):
    """(params, moments, accum, denom) of a golden case's inputs"""
    G = golden()
    params = {k: G[f"{tag}_in_{k}"] for k in GROUPS}
    moments = {k: (G[f"{tag}_in_{k}_exp_avg"], G[f"{tag}_in_{k}_exp_avg_sq"]) for k in GROUPS}
    return params, moments, G[f"{tag}_in_accum"], G[f"{tag}_in_denom"]


def check_against_golden(tag, got, got_m, n_copied, what=""):
    """got / got_m: new parameters and moments by name (numpy); rows below n_copied are copies, the rest children.  Copies and
    moments must be equal, children's xyz / scaling within TOL_CHILD.  -> {"xyz": max error, "scaling": max error}"""
    G = golden()
    err = {}
    for k in GROUPS:
        want = G[f"{tag}_out_{k}"]
        assert got[k].shape == want.shape, (what, k, got[k].shape, want.shape)
        if k in ("xyz", "scaling"):
            assert np.array_equal(got[k][:n_copied], want[:n_copied]), (what, k, "copied rows")
            err[k] = float(np.abs(got[k][n_copied:].astype(np.float64) - want[n_copied:]).max()) if len(want) > n_copied else 0.0
            print(f"{what} {tag} children {k}: max |error| {err[k]:.3e} (bound {TOL_CHILD:.0e})")
            assert err[k] <= TOL_CHILD, (what, k, err[k])
        else:
            assert np.array_equal(got[k], want), (what, k)
        for j, mk in enumerate(("exp_avg", "exp_avg_sq")):
            assert np.array_equal(got_m[k][j], G[f"{tag}_out_{k}_{mk}"]), (what, k, mk)
    return err
