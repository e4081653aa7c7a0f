"""The hash-grid encoding of InvUVNet (tiny-cuda-nn "HashGrid", F = 4), written out as float64 torch with autograd: the statement
tests/test_uvmap_*.py compare the HIP kernels (texture-gs_amd/csrc/uvmap.hip) against.  Restated from tiny-cuda-nn's published
grid encoding (UNPINNED against the package, like texgs.uvnet.unpack_tcnn_params).

Per level l: scale_l = exp2f(l * log2f(per_level_scale)) * base_res - 1 (float32), res_l = ceil(scale_l) + 1,
size_l = min(roundup8(res_l^3), 2^log2_T), offset_l = sum of the sizes before it.  Per point x (not clamped):
pos = scale_l x + 0.5, g = floor(pos), f = pos - g; corner p = g + c (uint32) -> p0 + p1 res + p2 res^2 when res^3 <= size,
else p0 ^ p1 * 2654435761 ^ p2 * 805459861 (uint32), then % size; enc[l*4 + j] = sum_c prod_d (c_d ? f_d : 1 - f_d) theta[...]."""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF
PRIMES = (1, 2654435761, 805459861)
SHIPPED = dict(n_levels=8, n_features=4, log2_hashmap_size=12, base_resolution=16.0, per_level_scale=1.447)
# Grids off the shipped one (fields not named are SHIPPED's) and the row count of every level.  With the shipped grid every level has
# 4096 rows, exactly the largest slab the backward accumulates in LDS (size * 16 B <= 64 KiB, csrc/uvmap.hip); these reach the
# rest: levels on the global-atomic path, both launches in one call, dense levels that are no power of two (roundup8(res^3)),
# L != 8, and a table so small that every point collides.
GRIDS = {
    "mixed": dict(n_levels=5, log2_hashmap_size=14),
    "small_dense": dict(n_levels=6, log2_hashmap_size=19, base_resolution=4.0, per_level_scale=1.5),
    "L16": dict(n_levels=16, log2_hashmap_size=10, base_resolution=2.0, per_level_scale=1.3),
    "L1": dict(n_levels=1),
    "tiny_hash": dict(n_levels=3, log2_hashmap_size=4, per_level_scale=2.0),
}
GRID_SIZES = {
    "mixed": [4096, 13824, 16384, 16384, 16384],                   # dense LDS; dense 24^3, global; hashed, global
    "small_dense": [64, 216, 736, 2744, 9264, 29792],              # 4^3, 6^3, 9^3 = 729, 14^3 in LDS; 21^3 = 9261, 31^3 = 29791 global
    "L16": [8, 32, 64, 128, 216, 512, 1000] + [1024] * 9,          # 2^3, 3^3 = 27, 4^3, 5^3 = 125, 6^3, 8^3, 10^3 dense, then hashed
    "L1": [4096],
    "tiny_hash": [16, 16, 16],
}


def _f32(v):
    return float(np.float32(v))


def levels(n_levels=8, n_features=4, log2_hashmap_size=12, base_resolution=16.0, per_level_scale=1.447):
    """[(scale, res, size, offset, hashed)] per level and the parameter count.  The fp32 scale: every operation rounded to
    float32 (log2 / exp2 evaluated in double and rounded once, i.e. correctly rounded, as the C library's log2f / exp2f are)."""
    assert n_features == 4
    lpls = _f32(math.log2(_f32(per_level_scale)))
    T = 1 << log2_hashmap_size
    out, off = [], 0
    for l in range(n_levels):
        s = _f32(_f32(_f32(2.0 ** _f32(_f32(l) * lpls)) * _f32(base_resolution)) - 1.0)
        res = int(math.ceil(s)) + 1
        size = min((res ** 3 + 7) // 8 * 8, T)
        out.append((s, res, size, off, res ** 3 > size))
        off += size
    return out, off * n_features


def _mul32(p, k):
    """(p * k) mod 2^32 for int64 tensors p < 2^32 without int64 overflow."""
    lo, hi = p & 0xFFFF, p >> 16
    return (lo * k + (((hi * k) & 0xFFFF) << 16)) & M32


def corner_index(p0, p1, p2, res, size, hashed):
    """Table row of corner p (int64 tensors or ints holding uint32 values) at a level."""
    t = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=torch.int64)
    p0, p1, p2 = t(p0) & M32, t(p1) & M32, t(p2) & M32
    if hashed:
        i = p0 ^ _mul32(p1, PRIMES[1]) ^ _mul32(p2, PRIMES[2])
    else:
        i = (p0 + p1 * res + p2 * (res * res)) & M32
    return i % size


def encode(x, params, cells=None, **grid):
    """enc float64 [N, L*4] of x [N, 3]; differentiable w.r.t. x and params (float64 copies).  `cells`: the fp32 points as a kernel
    sees them -- the cell of each point is then the one fp32 picks (pos rounded to float32 once, as fmaf does), the weights stay
    float64 (the encoding is continuous across a face, its x-gradient is not: this lines the two up where they straddle one)."""
    g = dict(SHIPPED, **grid)
    lv, n = levels(**g)
    assert params.numel() == n, (params.numel(), n)
    x = x.to(torch.float64)
    table = params.to(torch.float64).reshape(-1, 4)
    outs = []
    for (s, res, size, off, hashed) in lv:
        pos = x * s + 0.5
        if cells is None:
            fl = torch.floor(pos.detach())
        else:
            fl = torch.floor((cells.to(torch.float32).to(torch.float64) * s + 0.5).to(torch.float32).to(torch.float64)).to(x.device)
        f = pos - fl
        gi = fl.to(torch.int64) & M32
        acc = torch.zeros(x.shape[0], 4, dtype=torch.float64, device=x.device)
        for c in range(8):
            cc = (c & 1, (c >> 1) & 1, c >> 2)
            idx = corner_index(gi[:, 0] + cc[0], gi[:, 1] + cc[1], gi[:, 2] + cc[2], res, size, hashed)
            w = torch.ones(x.shape[0], dtype=torch.float64, device=x.device)
            for d in range(3):
                w = w * (f[:, d] if cc[d] else 1.0 - f[:, d])
            acc = acc + w[:, None] * table[off + idx]
        outs.append(acc)
    return torch.cat(outs, dim=1)


def face_distance(x, **grid):
    """Per point: the smallest distance (in cell units) of pos to a cell face over all levels and axes (float64)."""
    lv, _ = levels(**dict(SHIPPED, **grid))
    x = x.to(torch.float64)
    best = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=x.device)
    for (s, *_rest) in lv:
        pos = x * s + 0.5
        fr = pos - torch.floor(pos)
        best = torch.minimum(best, torch.minimum(fr, 1.0 - fr).min(dim=1).values)
    return best


def touch_sums(x, de, **grid):
    """per table entry: the sum over the (point, corner) terms that add into it of |d_enc|, and the number of those terms
    (float64, from the statement's corners)"""
    lv, n = levels(**dict(SHIPPED, **grid))
    out = torch.zeros(n // 4, 4, dtype=torch.float64)
    cnt = torch.zeros(n // 4, dtype=torch.int64)
    x = x.double()
    for l, (s, res, size, off, hashed) in enumerate(lv):
        gi = torch.floor(x * s + 0.5).long() & M32
        for c in range(8):
            idx = corner_index(gi[:, 0] + (c & 1), gi[:, 1] + ((c >> 1) & 1), gi[:, 2] + (c >> 2), res, size, hashed)
            out.index_add_(0, off + idx, de[:, 4 * l:4 * l + 4].abs().double())
            cnt.index_add_(0, off + idx, torch.ones_like(idx))
    return out.reshape(-1), cnt.repeat_interleave(4)


def rounding_bar(x_max=1.0, **grid):
    """E_F: the most a kernel's cell fraction f = pos - floor(pos) is off.  pos = fmaf(scale, x, 0.5) is rounded to fp32 once: half
    an ulp at |pos| <= pos_max = max_l scale_l * x_max + 0.5, i.e. 2^(floor(log2(pos_max)) - 24), plus 8 u (u = 2^-24) for the
    few fp32 operations after it.  The shipped grid with x_max = 1 has pos_max = 212.7: 2^-17 + 8 u."""
    lv, _ = levels(**dict(SHIPPED, **grid))
    pos_max = max(s for s, *_ in lv) * x_max + 0.5
    return 2.0 ** (math.floor(math.log2(pos_max)) - 24) + 8 * 2.0 ** -24
