"""The statement of the surface-point stage (include/texgs_surface.h, texgs/surface.py) in numpy, operation by operation: every
product, sum, difference and quotient below is ONE IEEE operation of the stated type, in the order the header lists them, so the
kernels of csrc/surface.hip (built without fused multiply-add) must give the same bits.

* `inverse_columns`  the float32 projection's inverse in float64, as adjugate over determinant (columns 0..2, twelve entries)
* `surface_points`   selection (alpha > threshold, strict), stable compaction in pixel order, and per selected pixel the fp64 clip
                     point times the inverse's columns, each component rounded to float32 once
* `compose`          out[c,p] = (bg[c] * (1 - alpha[p])) + (rank[p] >= 0 ? alpha[p] * values[rank[p]][c] : 0) in float32

tests/test_surface_host.py holds the points to the reference's own float64 result (tests/golden/host_terms.npz) and the compaction
and the composite to independent numpy; tests/test_surface_gpu.py holds the kernels equal to this file, bit for bit."""
import numpy as np

F = np.float32
D = np.float64
BACKGROUND = np.array([0.25, 0.5, 0.125], dtype=F)


def _t(p, q, r, u, v, w):
    return ((p * u) - (q * v)) + (r * w)


def inverse_columns(full_proj):
    """full_proj: 16 float32 (row-major, clip = [p, 1] @ P) -> float64 [4,3], entry [i,j] = B_ij of the inverse B"""
    a = [D(v) for v in np.asarray(full_proj, dtype=F).reshape(16)]
    a00, a01, a02, a03, a10, a11, a12, a13, a20, a21, a22, a23, a30, a31, a32, a33 = a
    with np.errstate(all="ignore"):
        s0 = a00 * a11 - a10 * a01
        s1 = a00 * a12 - a10 * a02
        s2 = a00 * a13 - a10 * a03
        s3 = a01 * a12 - a11 * a02
        s4 = a01 * a13 - a11 * a03
        s5 = a02 * a13 - a12 * a03
        c5 = a22 * a33 - a32 * a23
        c4 = a21 * a33 - a31 * a23
        c3 = a21 * a32 - a31 * a22
        c2 = a20 * a33 - a30 * a23
        c1 = a20 * a32 - a30 * a22
        c0 = a20 * a31 - a30 * a21
        det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
        B = np.empty((4, 3), D)
        B[0, 0] = _t(a11, a12, a13, c5, c4, c3) / det
        B[0, 1] = -_t(a01, a02, a03, c5, c4, c3) / det
        B[0, 2] = _t(a31, a32, a33, s5, s4, s3) / det
        B[1, 0] = -_t(a10, a12, a13, c5, c2, c1) / det
        B[1, 1] = _t(a00, a02, a03, c5, c2, c1) / det
        B[1, 2] = -_t(a30, a32, a33, s5, s2, s1) / det
        B[2, 0] = _t(a10, a11, a13, c4, c2, c0) / det
        B[2, 1] = -_t(a00, a01, a03, c4, c2, c0) / det
        B[2, 2] = _t(a30, a31, a33, s4, s2, s0) / det
        B[3, 0] = -_t(a10, a11, a12, c3, c1, c0) / det
        B[3, 1] = _t(a00, a01, a02, c3, c1, c0) / det
        B[3, 2] = -_t(a30, a31, a32, s3, s1, s0) / det
    return B


def world_points(depth, full_proj, zfar, znear):
    """Every pixel's point: depth f32 [H,W] -> f32 [H*W,3] (what the stage writes for the selected ones)"""
    d32 = np.asarray(depth, dtype=F)
    H, W = d32.shape
    B = inverse_columns(full_proj)
    zfar, znear = D(zfar), D(znear)
    with np.errstate(all="ignore"):
        d = d32.astype(D).reshape(-1)
        p = np.arange(H * W, dtype=np.int64)
        y, x = p // W, p % W
        nx = (2 * x + 1).astype(D) / D(W) - D(1)
        ny = (2 * y + 1).astype(D) / D(H) - D(1)
        zk = zfar - znear
        zb = (zfar * znear) / zk
        q0, q1 = nx * d, ny * d
        q2 = (zfar * d) / zk - zb
        out = np.empty((H * W, 3), F)
        for j in range(3):
            out[:, j] = (((q0 * B[0, j] + q1 * B[1, j]) + q2 * B[2, j]) + d * B[3, j]).astype(F)
    return out


def surface_points(depth, alpha, full_proj, zfar, znear, threshold=0.5):
    """-> dict(count, xyz f32 [M,3], index i64 [M], alpha f32 [M], rank i32 [H*W])"""
    a = np.asarray(alpha, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore"):
        sel = a > F(threshold)                              # strict, in float32: a NaN is not selected
    index = np.flatnonzero(sel).astype(np.int64)          # pixel order
    rank = np.full(a.size, -1, np.int32)
    rank[index] = np.arange(index.size, dtype=np.int32)
    xyz = world_points(depth, full_proj, zfar, znear)[index]
    return dict(count=int(index.size), xyz=np.ascontiguousarray(xyz), index=index, alpha=a[index].copy(), rank=rank)


def compose(values, rank, alpha, background=None):
    """values f32 [M,3], rank i32 [H*W] (or [H,W]), alpha f32 [H,W] -> f32 [3,H,W]"""
    a = np.asarray(alpha, dtype=F)
    H, W = a.shape[-2:]
    a = a.reshape(-1)
    rank = np.asarray(rank, dtype=np.int32).reshape(-1)
    values = np.asarray(values, dtype=F).reshape(-1, 3)
    bg = np.zeros(3, F) if background is None else np.asarray(background, dtype=F).reshape(3)
    on = rank >= 0
    out = np.empty((3, H * W), F)
    with np.errstate(all="ignore"):
        keep = F(1) - a
        for c in range(3):
            term = np.zeros(H * W, F)
            term[on] = a[on] * values[rank[on], c]
            out[c] = (bg[c] * keep) + term
    return out.reshape(3, H, W)


# ---- inputs the tests share ----
def camera(H, W, seed=0):
    """A pinhole camera looking at the origin from a seeded direction: (full_proj f32 [4,4] in the reference's row-vector convention,
    zfar, znear).  utils/graphics.py getProjectionMatrix / getWorld2View2 restated in numpy."""
    rng = np.random.default_rng(1000 + seed)
    zfar, znear = 100.0, 0.01
    fovx = 0.9
    fovy = 2 * np.arctan(np.tan(fovx / 2) * H / W) if W > 0 else fovx
    eye = rng.normal(size=3)
    eye = 3.0 * eye / np.linalg.norm(eye)
    fwd = -eye / np.linalg.norm(eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    Rwc = np.stack([right, up, fwd], axis=0)                # world -> camera rows
    view = np.eye(4)
    view[:3, :3] = Rwc
    view[:3, 3] = -Rwc @ eye
    tx, ty = np.tan(fovx / 2), np.tan(fovy / 2)
    Pm = np.zeros((4, 4))
    Pm[0, 0], Pm[1, 1] = 1 / tx, 1 / ty
    Pm[3, 2] = 1.0
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[2, 3] = -(zfar * znear) / (zfar - znear)
    full = (view.T.astype(F) @ Pm.T.astype(F)).astype(F)    # world_view_transform @ projection_matrix, both transposed (row vectors)
    return np.ascontiguousarray(full), zfar, znear


def make_depth(H, W, seed=0):
    rng = np.random.default_rng(2000 + seed)
    return (2.0 + 2.0 * rng.random((H, W))).astype(F)


def masks(H, W, B):
    """name -> alpha f32 [H,W]: the selections the GPU tests run (B = pixels per workgroup)"""
    n = H * W
    rng = np.random.default_rng(3000 + n)
    p = np.arange(n)
    lo, hi = F(0.25), F(0.75)
    out = {
        "none": np.full(n, lo, F),
        "all": np.full(n, hi, F),
        "first": np.where(p == 0, hi, lo).astype(F),
        "last": np.where(p == n - 1, hi, lo).astype(F),
        "alternate": np.where(p % 2 == 0, hi, lo).astype(F),
        "runs": np.where(((p + B // 2) // B) % 2 == 1, hi, lo).astype(F),        # runs of B from B/2: every workgroup border straddled
        "random": rng.random(n).astype(F),
    }
    special = np.array([0.5, np.nextafter(F(0.5), F(1)), np.nan, -0.0, np.inf, np.nextafter(F(0.5), F(0)), -np.inf, 1.0], dtype=F)
    out["special"] = special[rng.integers(0, special.size, n)] if n > special.size else np.resize(special, n)
    if n > special.size:
        out["special"][:special.size] = special             # each of them at least once
    return {k: v.reshape(H, W) for k, v in out.items()}
