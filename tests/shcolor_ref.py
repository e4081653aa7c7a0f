"""The colour stage (include/texgs_shcolor.h, csrc/shcolor_math.h) stated in numpy: spherical harmonics of degree 0..4 in a view
direction -> colour, what the reference's render glue does under `convert_SHs_python` (render/render.py:64-68 with utils/sh.py).

One class, two instances: S64 (float64, the truth the tests measure against) and S32 (float32, every operation rounded once, in the
operation order of the kernels -- the bit-exact contract).  Every expression below is written with explicit parentheses in the order
the header states; csrc/shcolor_math.h repeats them token for token.

    p = xyz - campos;  n = sqrt((px px + py py) + pz pz);  d = p / n                     (three divisions)
    b_k(d): the signed real SH basis, k < (deg + 1)^2                                     (basis() below)
    v_c = (((b_0 sh[0,c]) + b_1 sh[1,c]) + b_2 sh[2,c]) + ...                             (left to right)
    colour_c = (v_c + 0.5 < 0) ? 0 : v_c + 0.5                                            (a NaN stays a NaN)

Backward, per view in the order given, the sums starting at zero:
    g_c = (v_c + 0.5 >= 0) ? upstream_c : 0
    d_sh[k,c] = d_sh[k,c] + b_k * g_c
    t_k = ((g_0 sh[k,0]) + (g_1 sh[k,1])) + (g_2 sh[k,2])                                 k >= 1
    dd  = sum over k of grad b_k * t_k, in the order of dir_grad() below, starting at zero
    dot = ((dx ddx) + (dy ddy)) + (dz ddz);   d_xyz_i = d_xyz_i + (dd_i - (d_i dot)) / n
(degree 0 has no direction: d_xyz stays zero.)  `eval_sh` is the middle alone: the caller's directions, no +0.5, no clamp, no gate,
d_dirs = 0 + dd."""
import numpy as np

F, D = np.float32, np.float64
PARITY_FACTOR = 4.0             # the ratio rule of tests/test_params_gpu.py
PARITY_FLOOR = 2.0 ** -24

# the real SH constants of utils/sh.py (Python floats there: rounded to the working type before use)
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
      0.47308734787878004, -1.7701307697799304, 0.6258357354491761]
COEFFS = (1, 4, 9, 16, 25)


class Statement:
    def __init__(self, T):
        self.T = T
        self.c0, self.c1 = T(C0), T(C1)
        self.c2, self.c3, self.c4 = [T(c) for c in C2], [T(c) for c in C3], [T(c) for c in C4]

    def n(self, v):
        return self.T(v)

    def const_like(self, x, c):
        return np.full(x.shape, c, self.T)

    def direction(self, xyz, campos):
        T = self.T
        p = np.asarray(xyz, T) - np.asarray(campos, T).reshape(1, 3)
        with np.errstate(all="ignore"):
            n = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
            d = np.stack([p[:, 0] / n, p[:, 1] / n, p[:, 2] / n], axis=1)
        return d, n

    def basis(self, deg, x, y, z):
        """The signed basis: b[k] * sh[k] are the terms of utils/sh.py:74-111, each product chain left to right"""
        n = self.n
        c0, c1, c2, c3, c4 = self.c0, self.c1, self.c2, self.c3, self.c4
        b = [self.const_like(x, c0)]
        if deg >= 1:
            b += [-(c1 * y), c1 * z, -(c1 * x)]
        if deg >= 2:
            xx, yy, zz = x * x, y * y, z * z
            xy, yz, xz = x * y, y * z, x * z
            b += [c2[0] * xy,
                  c2[1] * yz,
                  c2[2] * (((n(2) * zz) - xx) - yy),
                  c2[3] * xz,
                  c2[4] * (xx - yy)]
        if deg >= 3:
            b += [(c3[0] * y) * ((n(3) * xx) - yy),
                  (c3[1] * xy) * z,
                  (c3[2] * y) * (((n(4) * zz) - xx) - yy),
                  (c3[3] * z) * (((n(2) * zz) - (n(3) * xx)) - (n(3) * yy)),
                  (c3[4] * x) * (((n(4) * zz) - xx) - yy),
                  (c3[5] * z) * (xx - yy),
                  (c3[6] * x) * (xx - (n(3) * yy))]
        if deg >= 4:
            b += [(c4[0] * xy) * (xx - yy),
                  (c4[1] * yz) * ((n(3) * xx) - yy),
                  (c4[2] * xy) * ((n(7) * zz) - n(1)),
                  (c4[3] * yz) * ((n(7) * zz) - n(3)),
                  c4[4] * ((zz * ((n(35) * zz) - n(30))) + n(3)),
                  (c4[5] * xz) * ((n(7) * zz) - n(3)),
                  (c4[6] * (xx - yy)) * ((n(7) * zz) - n(1)),
                  (c4[7] * xz) * (xx - (n(3) * yy)),
                  c4[8] * ((xx * (xx - (n(3) * yy))) - (yy * ((n(3) * xx) - yy)))]
        return b

    def dir_grad(self, deg, x, y, z, t):
        """dd = sum_k grad b_k * t[k], the terms that are not identically zero, in this order, each sum starting at zero"""
        n = self.n
        c1, c2, c3, c4 = self.c1, self.c2, self.c3, self.c4
        zero = np.zeros(x.shape, self.T)
        ddx, ddy, ddz = zero, zero, zero
        if deg >= 1:
            ddy = ddy + (-c1) * t[1]
            ddz = ddz + c1 * t[2]
            ddx = ddx + (-c1) * t[3]
        if deg >= 2:
            ddx = ddx + (c2[0] * y) * t[4]
            ddy = ddy + (c2[0] * x) * t[4]
            ddy = ddy + (c2[1] * z) * t[5]
            ddz = ddz + (c2[1] * y) * t[5]
            ddx = ddx + (c2[2] * (n(-2) * x)) * t[6]
            ddy = ddy + (c2[2] * (n(-2) * y)) * t[6]
            ddz = ddz + (c2[2] * (n(4) * z)) * t[6]
            ddx = ddx + (c2[3] * z) * t[7]
            ddz = ddz + (c2[3] * x) * t[7]
            ddx = ddx + (c2[4] * (n(2) * x)) * t[8]
            ddy = ddy + (c2[4] * (n(-2) * y)) * t[8]
        if deg >= 3:
            xx, yy, zz = x * x, y * y, z * z
            xy, yz, xz = x * y, y * z, x * z
            ddx = ddx + (c3[0] * (n(6) * xy)) * t[9]
            ddy = ddy + (c3[0] * ((n(3) * xx) - (n(3) * yy))) * t[9]
            ddx = ddx + (c3[1] * yz) * t[10]
            ddy = ddy + (c3[1] * xz) * t[10]
            ddz = ddz + (c3[1] * xy) * t[10]
            ddx = ddx + (c3[2] * (n(-2) * xy)) * t[11]
            ddy = ddy + (c3[2] * (((n(4) * zz) - xx) - (n(3) * yy))) * t[11]
            ddz = ddz + (c3[2] * (n(8) * yz)) * t[11]
            ddx = ddx + (c3[3] * (n(-6) * xz)) * t[12]
            ddy = ddy + (c3[3] * (n(-6) * yz)) * t[12]
            ddz = ddz + (c3[3] * (((n(6) * zz) - (n(3) * xx)) - (n(3) * yy))) * t[12]
            ddx = ddx + (c3[4] * (((n(4) * zz) - (n(3) * xx)) - yy)) * t[13]
            ddy = ddy + (c3[4] * (n(-2) * xy)) * t[13]
            ddz = ddz + (c3[4] * (n(8) * xz)) * t[13]
            ddx = ddx + (c3[5] * (n(2) * xz)) * t[14]
            ddy = ddy + (c3[5] * (n(-2) * yz)) * t[14]
            ddz = ddz + (c3[5] * (xx - yy)) * t[14]
            ddx = ddx + (c3[6] * ((n(3) * xx) - (n(3) * yy))) * t[15]
            ddy = ddy + (c3[6] * (n(-6) * xy)) * t[15]
        if deg >= 4:
            xyz = xy * z
            ddx = ddx + ((c4[0] * y) * ((n(3) * xx) - yy)) * t[16]
            ddy = ddy + ((c4[0] * x) * (xx - (n(3) * yy))) * t[16]
            ddx = ddx + (c4[1] * (n(6) * xyz)) * t[17]
            ddy = ddy + ((c4[1] * z) * ((n(3) * xx) - (n(3) * yy))) * t[17]
            ddz = ddz + ((c4[1] * y) * ((n(3) * xx) - yy)) * t[17]
            ddx = ddx + ((c4[2] * y) * ((n(7) * zz) - n(1))) * t[18]
            ddy = ddy + ((c4[2] * x) * ((n(7) * zz) - n(1))) * t[18]
            ddz = ddz + (c4[2] * (n(14) * xyz)) * t[18]
            ddy = ddy + ((c4[3] * z) * ((n(7) * zz) - n(3))) * t[19]
            ddz = ddz + ((c4[3] * y) * ((n(21) * zz) - n(3))) * t[19]
            ddz = ddz + ((c4[4] * z) * ((n(140) * zz) - n(60))) * t[20]
            ddx = ddx + ((c4[5] * z) * ((n(7) * zz) - n(3))) * t[21]
            ddz = ddz + ((c4[5] * x) * ((n(21) * zz) - n(3))) * t[21]
            ddx = ddx + ((c4[6] * (n(2) * x)) * ((n(7) * zz) - n(1))) * t[22]
            ddy = ddy + ((c4[6] * (n(-2) * y)) * ((n(7) * zz) - n(1))) * t[22]
            ddz = ddz + ((c4[6] * (xx - yy)) * (n(14) * z)) * t[22]
            ddx = ddx + ((c4[7] * z) * ((n(3) * xx) - (n(3) * yy))) * t[23]
            ddy = ddy + (c4[7] * (n(-6) * xyz)) * t[23]
            ddz = ddz + ((c4[7] * x) * (xx - (n(3) * yy))) * t[23]
            ddx = ddx + ((c4[8] * (n(4) * x)) * (xx - (n(3) * yy))) * t[24]
            ddy = ddy + ((c4[8] * (n(4) * y)) * (yy - (n(3) * xx))) * t[24]
        return ddx, ddy, ddz

    # ---- forward ----
    def _eval(self, deg, sh, d):
        """sh [N,K,3], d [N,3] -> (v [N,3], basis)"""
        with np.errstate(all="ignore"):
            b = self.basis(deg, d[:, 0], d[:, 1], d[:, 2])
            v = b[0][:, None] * sh[:, 0, :]
            for k in range(1, len(b)):
                v = v + b[k][:, None] * sh[:, k, :]
        return v, b

    def eval_sh(self, deg, sh, dirs):
        """The reference's eval_sh on coefficients laid out [N,K,3] (its sh[..., c, k] is sh[:, k, c] here)"""
        return self._eval(deg, np.asarray(sh, self.T), np.asarray(dirs, self.T))[0]

    def clamp(self, v):
        with np.errstate(all="ignore"):
            w = v + self.T(0.5)
            return np.where(w < 0, self.T(0), w)

    def colors(self, deg, sh, xyz, campos):
        """render.py:64-68 for one camera -> [N,3]"""
        sh = np.asarray(sh, self.T)
        if deg == 0:
            d = np.zeros((sh.shape[0], 3), self.T)
        else:
            d, _ = self.direction(xyz, campos)
        return self.clamp(self._eval(deg, sh, d)[0])

    def colors_views(self, deg, sh, xyz, camposes):
        return np.stack([self.colors(deg, sh, xyz, c) for c in np.asarray(camposes, self.T).reshape(-1, 3)])

    # ---- backward ----
    def _view_backward(self, deg, sh, d, g, gated, d_sh, want_dd):
        T = self.T
        with np.errstate(all="ignore"):
            v, b = self._eval(deg, sh, d)
            if gated:
                g = np.where(v + T(0.5) >= 0, g, T(0))
            for k in range(len(b)):
                d_sh[:, k, :] = d_sh[:, k, :] + b[k][:, None] * g
            if deg == 0 or not want_dd:
                return None
            t = [None] + [((g[:, 0] * sh[:, k, 0]) + (g[:, 1] * sh[:, k, 1])) + (g[:, 2] * sh[:, k, 2]) for k in range(1, len(b))]
            return self.dir_grad(deg, d[:, 0], d[:, 1], d[:, 2], t)

    def eval_sh_backward(self, deg, sh, dirs, g):
        """-> (d_sh [N,K,3], d_dirs [N,3]); coefficients beyond the degree get zero"""
        T = self.T
        sh, d, g = np.asarray(sh, T), np.asarray(dirs, T), np.asarray(g, T)
        d_sh = np.zeros_like(sh)
        dd = self._view_backward(deg, sh, d, g, False, d_sh, True)
        d_dirs = np.zeros_like(d)
        if dd is not None:
            with np.errstate(all="ignore"):
                d_dirs = d_dirs + np.stack(dd, axis=1)
        return d_sh, d_dirs

    def colors_backward(self, deg, sh, xyz, camposes, g):
        """camposes [V,3], g [V,N,3] -> (d_sh [N,K,3], d_xyz [N,3]): the views summed in the order given"""
        T = self.T
        sh, xyz, g = np.asarray(sh, T), np.asarray(xyz, T), np.asarray(g, T)
        cams = np.asarray(camposes, T).reshape(-1, 3)
        d_sh, d_xyz = np.zeros_like(sh), np.zeros_like(xyz)
        for v in range(cams.shape[0]):
            if deg == 0:
                d, n = np.zeros_like(xyz), None
            else:
                d, n = self.direction(xyz, cams[v])
            dd = self._view_backward(deg, sh, d, g[v], True, d_sh, True)
            if dd is None:
                continue
            with np.errstate(all="ignore"):
                dot = ((d[:, 0] * dd[0]) + (d[:, 1] * dd[1])) + (d[:, 2] * dd[2])
                for i in range(3):
                    d_xyz[:, i] = d_xyz[:, i] + (dd[i] - (d[:, i] * dot)) / n
        return d_sh, d_xyz


S64, S32 = Statement(D), Statement(F)


class _TorchStatement(Statement):
    """The same table of basis functions on torch tensors, the constants as Python floats: what the glue's torch chain computes"""

    def __init__(self):
        super().__init__(float)

    def const_like(self, x, c):
        import torch
        return torch.full_like(x, c)


def torch_lines(features, xyz, campos, deg):
    """The `convert_SHs_python` branch of the render glue (render/render.py:64-68) as a chain of elementwise torch operations under
    autograd, in whatever dtype and on whatever device the tensors have: the transposed coefficient view, the offset from the camera
    centre over its norm, the SH polynomials term by term on [N,1] columns broadcast against [N,3] coefficients, + 0.5, clamp at
    zero.  The comparison leg of the GPU tests and of scripts/bench_shcolor.py."""
    import torch
    K = features.shape[1]
    view = features.transpose(1, 2).view(-1, 3, K)
    offset = xyz - campos.reshape(1, 3).repeat(features.shape[0], 1)
    d = offset / offset.norm(dim=1, keepdim=True)
    b = _TorchStatement().basis(deg, d[:, 0:1], d[:, 1:2], d[:, 2:3])
    val = C0 * view[..., 0]
    for k in range(1, len(b)):
        val = val + b[k] * view[..., k]
    return torch.clamp_min(val + 0.5, 0.0)


def random_case(N, K, seed, V=1):
    """Standard-normal coefficients, points a few units from cameras near the origin, upstream gradients of order one"""
    rng = np.random.default_rng(seed)
    sh = rng.standard_normal((N, K, 3)).astype(F)
    u = rng.standard_normal((N, 3))
    xyz = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (N, 1))).astype(F)
    cams = rng.uniform(-1.0, 1.0, (V, 3)).astype(F)
    g = rng.standard_normal((V, N, 3)).astype(F)
    return sh, xyz, cams, g


def max_error(got, want64, scale):
    """max |got - want64| / scale over every element (scale broadcasts; an element whose scale is 0 must be exact)"""
    got, want64 = np.asarray(got).astype(D), np.asarray(want64, D)
    got = got.reshape(want64.shape)
    scale = np.broadcast_to(np.asarray(scale, D), want64.shape)
    err = np.abs(got - want64)
    with np.errstate(all="ignore"):
        rel = np.where(err == 0, 0.0, np.where(scale > 0, err / scale, np.inf))
    assert not np.isnan(rel).any()
    return float(rel.max()) if rel.size else 0.0


def backward_scales(deg, sh, xyz, cams, g):
    """The scales the backward's parity bound is stated in: what the sums are made of, not what survives their cancellation.
    d_sh[k,c]: sum over views of |b_k| |g_c|;  d_xyz, per row: sum over views of sum_k |grad b_k|_1 (|g_0 sh[k,0]| + |g_1 sh[k,1]| +
    |g_2 sh[k,2]|) / n, the terms of dd by magnitude (the projection mixes the components, so a row has one scale).  Upstream
    gradients are taken ungated: the float32 and float64 gates may differ in a row whose v + 0.5 is within rounding of zero."""
    sh, xyz, g = np.asarray(sh, D), np.asarray(xyz, D), np.asarray(g, D)
    cams = np.asarray(cams, D).reshape(-1, 3)
    N = xyz.shape[0]
    s_sh = np.zeros_like(sh)
    s_xyz = np.zeros((N, 1))
    A = (deg + 1) ** 2
    for v in range(cams.shape[0]):
        d, n = S64.direction(xyz, cams[v])
        if deg == 0:
            d = np.zeros_like(xyz)
        b = S64.basis(deg, d[:, 0], d[:, 1], d[:, 2])
        for k in range(A):
            s_sh[:, k, :] += np.abs(b[k])[:, None] * np.abs(g[v])
        for k in range(1, A):
            one_hot = [np.ones(N) if j == k else np.zeros(N) for j in range(A)]
            gb = S64.dir_grad(deg, d[:, 0], d[:, 1], d[:, 2], one_hot)          # grad b_k
            t = (np.abs(g[v]) * np.abs(sh[:, k, :])).sum(axis=1)
            s_xyz[:, 0] += (np.abs(gb[0]) + np.abs(gb[1]) + np.abs(gb[2])) * t / n
    return s_sh, s_xyz


def same_class_and_bits(a, b):
    """zero / infinity / NaN in the same places, and equal bits where finite (so the sign of a zero counts)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])
