"""The statement of seamless cubemap sampling (texgs.cubetex, csrc/cubetex.hip) in float64 torch, differentiable.

Layouts: texture [6, R, R, C] (faces +x, -x, +y, -y, +z, -z, channels last), directions [N, 3] of any length, result [N, C].
The face is the dominant axis (`>=` tie order x, y, z), col = (sc/ma + 1) R/2 - 0.5 and row likewise, texel centres at
(i + 0.5)/R: NVDIFFREC/util.py:94-101 `cube_to_dir` inverted (tests/golden/cube.npz pins it).

`linear`: four bilinear taps around (floor(col), floor(row)).  A tap inside the face reads it.  A tap with one coordinate out of
range (at -1 or R) reads the face across that edge.  A tap with both out of range is a cube corner, where no fourth texel exists:
it is dropped and the other three weights are divided by their sum.

The neighbour across an edge is found GEOMETRICALLY here: the out-of-range tap's centre (|s| or |t| = 1 + 1/R) goes through
`cube_to_dir` and the ordinary face selection, and the nearest texel of the face it lands on is the tap.  In float64 that is
unambiguous: the centre's offset from a texel centre along the edge stays below 0.5 R/(R + 1) texel.  The kernel reaches the same
texel from an integer table, so the two routes are independent.
"""
import math

import torch

SH_C0 = 0.28209479177387814

# cube_to_dir(face, x, y) = M[face] @ (x, y, 1)      (NVDIFFREC/util.py:94-101)
_M = torch.tensor([
    [[0, 0, 1], [0, -1, 0], [-1, 0, 0]],
    [[0, 0, -1], [0, -1, 0], [1, 0, 0]],
    [[1, 0, 0], [0, 0, 1], [0, 1, 0]],
    [[1, 0, 0], [0, 0, -1], [0, -1, 0]],
    [[1, 0, 0], [0, -1, 0], [0, 0, 1]],
    [[-1, 0, 0], [0, -1, 0], [0, 0, -1]],
], dtype=torch.float64)


def sh02rgb(t):
    return torch.clamp(SH_C0 * t + 0.5, 0.0, 1.0)


def cube_to_dir(face, s, t):
    """face int64 [...], s / t float64 [...] -> [..., 3]"""
    v = torch.stack([s, t, torch.ones_like(s)], -1)
    return torch.einsum("...ij,...j->...i", _M[face], v)


def address(d, R):
    """d float64 [N, 3] (finite, non-zero) -> face int64 [N], col, row float64 [N] (differentiable in d)"""
    a = d.abs()
    fx = (a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2])
    fy = ~fx & (a[:, 1] >= a[:, 2])
    axis = torch.where(fx, 0, torch.where(fy, 1, 2))
    m = d.gather(1, axis[:, None])[:, 0]
    face = 2 * axis + (m < 0).long()
    # (s, t, 1) = M[face]^T d / |m|: every M[face] is a signed permutation, so its transpose is its inverse
    st = torch.einsum("nji,nj->ni", _M[face], d) / m.abs()[:, None]
    half = 0.5 * R
    return face, (st[:, 0] + 1.0) * half - 0.5, (st[:, 1] + 1.0) * half - 0.5


def nearest_texel(d, R):
    face, col, row = address(d, R)
    x = torch.floor(col + 0.5).long().clamp(0, R - 1)
    y = torch.floor(row + 0.5).long().clamp(0, R - 1)
    return face, x, y


def resolve_tap(face, x, y, R):
    """Tap (x, y) of `face` with x, y in [-1, R] -> (face', x', y', valid): itself inside the face, the neighbour's texel across
    an edge (by geometry), invalid at a cube corner."""
    ox = (x < 0) | (x >= R)
    oy = (y < 0) | (y >= R)
    valid = ~(ox & oy)
    s = (x.double() + 0.5) * (2.0 / R) - 1.0
    t = (y.double() + 0.5) * (2.0 / R) - 1.0
    nf, nx, ny = nearest_texel(cube_to_dir(face, s, t), R)
    cross = ox ^ oy
    return (torch.where(cross, nf, face), torch.where(cross, nx, x.clamp(0, R - 1)), torch.where(cross, ny, y.clamp(0, R - 1)),
            valid)


def degenerate(dirs):
    return ~torch.isfinite(dirs).all(-1) | (dirs == 0).all(-1)


def sample(tex, dirs, filter="linear", tap_map=False, touching_abs=None, return_taps=False):
    """tex [6, R, R, C], dirs [N, 3] -> float64 [N, C].  tap_map: sh02rgb on every tap before the filter.
    touching_abs: g [N, C] -> additionally, per texel, the sum of |g| over the queries that have a tap on it, [6, R, R, C] (what the
    rounding error of the texture gradient is bounded by).
    return_taps: additionally int64 [N, 4] (taps 00, 10, 01, 11): 0 a tap on the query's own face, 1 + edge (0: x = -1, 1: x = R,
    2: y = -1, 3: y = R) a tap across that edge, -1 the dropped corner tap."""
    tex = tex.double()
    dirs = dirs.double()
    R, C = tex.shape[1], tex.shape[3]
    bad = degenerate(dirs)
    d = torch.where(bad[:, None], torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64), dirs)
    if tap_map:
        tex = sh02rgb(tex)
    flat = tex.reshape(-1, C)
    if filter == "nearest":
        f, x, y = nearest_texel(d, R)
        out = flat[(f * R + y) * R + x]
        return out * (~bad)[:, None]
    assert filter == "linear"
    face, col, row = address(d, R)
    x0 = torch.floor(col.detach()).clamp(-1, R - 1)
    y0 = torch.floor(row.detach()).clamp(-1, R - 1)
    fx, fy = col - x0, row - y0
    num = torch.zeros(d.shape[0], C, dtype=torch.float64)
    den = torch.zeros(d.shape[0], dtype=torch.float64)
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            w = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
            tf, tx, ty, valid = resolve_tap(face, x0.long() + i, y0.long() + j, R)
            w = w * valid
            idx = (tf * R + ty) * R + tx
            num = num + w[:, None] * flat[idx]
            den = den + w
            xi, yi = x0.long() + i, y0.long() + j
            ox, oy = (xi < 0) | (xi >= R), (yi < 0) | (yi >= R)
            kind = torch.where(ox & oy, -1, torch.where(ox, torch.where(xi < 0, 1, 2), torch.where(oy, torch.where(yi < 0, 3, 4), 0)))
            taps.append((idx, valid, kind))
    out = num / den[:, None] * (~bad)[:, None]
    res = [out]
    if touching_abs is not None:
        acc = torch.zeros(6 * R * R, C, dtype=torch.float64)
        g = touching_abs.double().abs() * (~bad)[:, None]
        for idx, valid, _ in taps:
            acc.index_add_(0, idx, valid[:, None] * g)
        res.append(acc.reshape(6, R, R, C))
    if return_taps:
        res.append(torch.stack([k for _, _, k in taps], 1))
    return res[0] if len(res) == 1 else tuple(res)


def latlong_dirs(resolution):
    """float64 [H, W, 3]: the directions of NVDIFFREC/util.py:119-133 cubemap_to_latlong ('ij' meshgrid: gy runs over rows)"""
    H, W = resolution
    gy = torch.linspace(1.0 / H, 1.0 - 1.0 / H, H, dtype=torch.float64)
    gx = torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, dtype=torch.float64)
    gy, gx = torch.meshgrid(gy, gx, indexing="ij")
    st, ct = torch.sin(gy * math.pi), torch.cos(gy * math.pi)
    sp, cp = torch.sin(gx * math.pi), torch.cos(gx * math.pi)
    return torch.stack([st * sp, ct, -st * cp], -1)


def chessboard(resolution=6, cell=16):
    """float64 [6, 16 r, 16 r, 3]: models/uv_map_gaussian3d.py:249-260, the board of chessboard_texture"""
    board = torch.zeros(6, resolution * cell, resolution * cell, 3, dtype=torch.float64)
    for i in range(resolution):                 # the reference's loop, cell by cell
        for j in range(resolution):
            colour = [0.0, 1.0, 1.0] if (i + j) % 2 == 0 else [1.0, 0.0, 0.0]
            board[:, i * cell:(i + 1) * cell, j * cell:(j + 1) * cell, :] = torch.tensor(colour, dtype=torch.float64)
    return board
