"""The statement texgs.points is tested against, three times, and the seeded clouds of the point tests.

For fp32 points a, b:  dx = a.x - b.x; dy = a.y - b.y; dz = a.z - b.z; d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded
to fp32 (no fused multiply-add).

* 3-NN: mean_d2[i] = ((b0 + b1) + b2) / 3, b0 <= b1 <= b2 the three smallest d2(x_i, x_j) over j != i (excluded by INDEX).
* FPS:  idx[0] = start; m[j] = +inf; for t = 1 .. K-1: m[j] = min(m[j], d2(x_j, x_idx[t-1])); idx[t] = argmax_j m[j], the lowest j
  on ties.

Forms: numpy fp32 (op by op), float64 (the same formulas in double), and torch fp32 with one torch op per arithmetic operation
(no addcmul, no cdist, no compile) so that it can run on the device for the large cases.  The torch form divides by 3 on the host:
IEEE division is certain there.
"""
import numpy as np
import torch

F32 = np.float32


# ---- numpy ------------------------------------------------------------------------------------------------------------------------

def _d2_rows_np(p, lo, hi, dtype):
    """[hi - lo, N] squared distances of rows lo..hi to all rows, op by op in `dtype`"""
    a = p[lo:hi, None, :].astype(dtype)
    b = p[None, :, :].astype(dtype)
    dx = a[..., 0] - b[..., 0]
    dy = a[..., 1] - b[..., 1]
    dz = a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def knn3_np(points, dtype=F32, chunk=512):
    """the 3-NN statement in `dtype` (np.float32: the contract; np.float64: the yardstick of its rounding error)"""
    p = np.ascontiguousarray(np.asarray(points, dtype=F32))
    n = p.shape[0]
    assert n >= 4
    out = np.empty(n, dtype=dtype)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = _d2_rows_np(p, lo, hi, dtype)
        d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
        out[lo:hi] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / dtype(3.0)
    return out


def fps_np(points, k, start=0, dtype=F32):
    p = np.ascontiguousarray(np.asarray(points, dtype=F32)).astype(dtype)
    n = p.shape[0]
    assert 1 <= k <= n and 0 <= start < n
    idx = np.empty(k, dtype=np.int64)
    idx[0] = start
    m = np.full(n, np.inf, dtype=dtype)
    for t in range(1, k):
        q = p[idx[t - 1]]
        dx = p[:, 0] - q[0]
        dy = p[:, 1] - q[1]
        dz = p[:, 2] - q[2]
        m = np.minimum(m, (dx * dx + dy * dy) + dz * dz)
        idx[t] = int(np.argmax(m))          # numpy: the first occurrence of the maximum = the lowest index
    return idx


# ---- torch fp32, one op per arithmetic operation ---------------------------------------------------------------------------------

def knn3_torch(points, chunk=512):
    """fp32 3-NN statement on points.device -> float32 [N] on the CPU"""
    p = points.detach().to(torch.float32).contiguous()
    n = p.shape[0]
    assert n >= 4
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    sums = torch.empty(n, dtype=torch.float32, device=p.device)
    rows = torch.arange(n, device=p.device)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=p.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        dx = torch.sub(x[lo:hi, None], x[None, :])
        dy = torch.sub(y[lo:hi, None], y[None, :])
        dz = torch.sub(z[lo:hi, None], z[None, :])
        xx = torch.mul(dx, dx)
        yy = torch.mul(dy, dy)
        zz = torch.mul(dz, dz)
        d = torch.add(torch.add(xx, yy), zz)
        d[rows[: hi - lo], rows[lo:hi]] = inf
        b = torch.topk(d, 3, dim=1, largest=False, sorted=True).values       # a set property: ties do not matter
        sums[lo:hi] = torch.add(torch.add(b[:, 0], b[:, 1]), b[:, 2])
    return torch.div(sums.cpu(), torch.tensor(3.0, dtype=torch.float32))


def fps_torch(points, k, start=0):
    """fp32 FPS statement on points.device -> int64 [K] on the CPU.  The pick is written as `first index where m equals its
    maximum`, which is the lowest index on ties on any device."""
    p = points.detach().to(torch.float32).contiguous()
    n = p.shape[0]
    assert 1 <= k <= n and 0 <= start < n
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    idx = [int(start)]
    m = torch.full((n,), float("inf"), dtype=torch.float32, device=p.device)
    for _ in range(1, k):
        j = idx[-1]
        dx = torch.sub(x, x[j])
        dy = torch.sub(y, y[j])
        dz = torch.sub(z, z[j])
        d = torch.add(torch.add(torch.mul(dx, dx), torch.mul(dy, dy)), torch.mul(dz, dz))
        m = torch.minimum(m, d)
        idx.append(int(torch.nonzero(m == m.max())[0, 0]))
    return torch.tensor(idx, dtype=torch.int64)


# ---- clouds -----------------------------------------------------------------------------------------------------------------------

def uniform(n, seed):
    """unit cube"""
    return np.random.default_rng(seed).random((n, 3), dtype=F32)


def clustered(n, seed):
    """12 Gaussian clusters (centres in [-4, 4]^3) with per-point spreads drawn from {1e-3, 0.02, 0.3}, 1 % outliers at sigma = 60,
    2 % exact duplicates of other points of the cloud"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-4.0, 4.0, (12, 3))
    which = rng.integers(0, 12, n)
    spread = rng.choice(np.array([1e-3, 0.02, 0.3]), n)
    p = centres[which] + rng.standard_normal((n, 3)) * spread[:, None]
    n_out = max(1, n // 100)
    out = rng.choice(n, n_out, replace=False)
    p[out] = rng.standard_normal((n_out, 3)) * 60.0
    p = p.astype(F32)
    n_dup = max(1, n // 50)
    dst = rng.choice(n, n_dup, replace=False)
    src = rng.integers(0, n, n_dup)
    p[dst] = p[src]
    return np.ascontiguousarray(p)


def on_line(n, seed):
    """all points on a line parallel to x: two axes of zero extent"""
    p = np.zeros((n, 3), dtype=F32)
    p[:, 0] = np.random.default_rng(seed).random(n, dtype=F32) * F32(10.0)
    p[:, 1] = F32(0.25)
    p[:, 2] = F32(-3.0)
    return p


def on_plane(n, seed):
    p = np.random.default_rng(seed).random((n, 3), dtype=F32)
    p[:, 2] = F32(1.5)
    return p


def identical(n):
    return np.full((n, 3), 0.7, dtype=F32)


def one_repeated(n, repeats, seed):
    """n points, one of them present `repeats` times"""
    p = uniform(n, seed)
    rng = np.random.default_rng(seed + 1)
    where = rng.choice(n, repeats, replace=False)
    p[where] = p[where[0]]
    return p


def cube_corners():
    return np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=F32)
