"""The arithmetic of the parameter stage (include/texgs_params.h, csrc/params_math.h) stated in numpy: once in float64 -- the truth
the tests measure errors against, with numpy's own exp and log -- and once in float32 with the operation order of the kernels, exp
and log included (the two polynomials of the header), so that the device can be compared with it bit for bit.

    S = Statement(np.float64)   or   Statement(np.float32)
    S.activate(scaling, rotation, opacity, epsilon=None) -> dict(scales, rotations, opacities[, terms, reg])
    S.activate_backward(rotation, scales, opacities, g_scales, g_rotations, g_opacities, g_reg, epsilon) -> (d_scaling, d_rotation, d_opacity)
    S.covariance(scaling, rotation, modifier) -> [N,6];   S.covariance_backward(scaling, rotation, modifier, g_cov) -> (d_scaling, d_rotation)
Upstream gradients that are None are zero.  Everything is vectorised over rows; nothing here depends on N or on a row's position
except the regulariser's mean."""
import numpy as np

F = np.float32
D = np.float64
NORM_EPS = 1e-12


def exp32(x):
    """exp of the header, float32, every operation rounded once"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        nan = np.isnan(x)
        xc = np.where(nan, F(0), x)
        xc = np.where(xc < F(-110), F(-110), np.where(xc > F(90), F(90), xc)).astype(F)
        k = np.rint(xc * F(1.44269504))
        r = (xc - k * F(0.693359375)) - k * F(-2.12194440e-4)
        p = F(1.9875691500e-4) * r + F(1.3981999507e-3)
        p = p * r + F(8.3334519073e-3)
        p = p * r + F(4.1665795894e-2)
        p = p * r + F(1.6666665459e-1)
        p = p * r + F(5.0000001201e-1)
        out = np.ldexp((p * (r * r) + r) + F(1), k.astype(np.int32))
    assert out.dtype == F
    return np.where(nan, x, out)


def log32(v):
    """log of the header for positive finite float32"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        m, e = np.frexp(v)
        low = m < F(0.707106781186547524)
        e = np.where(low, e - 1, e)
        m = np.where(low, (m + m) - F(1), m - F(1)).astype(F)
        z = m * m
        y = F(7.0376836292e-2) * m + F(-1.1514610310e-1)
        for c in (1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1,
                  3.3333331174e-1):
            y = y * m + F(c)
        y = (y * m) * z
        fe = e.astype(F)
        y = y + F(-2.12194440e-4) * fe
        y = y - F(0.5) * z
        out = (m + y) + F(0.693359375) * fe
    assert out.dtype == F
    return out


class Statement:
    def __init__(self, dtype):
        self.T = np.dtype(dtype).type
        assert self.T in (F, D)
        self.exp = exp32 if self.T is F else np.exp
        self.log = log32 if self.T is F else np.log

    def _a(self, x):
        return None if x is None else np.asarray(x).astype(self.T)

    def norm(self, q):
        return np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])

    def sigmoid(self, x):
        T = self.T
        return T(1) / (T(1) + self.exp(-x))

    def clamp(self, o, eps):
        T = self.T
        e, hi = T(eps), T(1) - T(eps)
        return np.where(o < e, e, np.where(o > hi, hi, o)).astype(T)

    def activate(self, scaling, rotation, opacity, epsilon=None):
        T = self.T
        a, q, x = self._a(scaling), self._a(rotation), self._a(opacity).reshape(-1)
        with np.errstate(all="ignore"):
            n = self.norm(q)
            d = np.where(n < T(NORM_EPS), T(NORM_EPS), n)
            out = {"scales": self.exp(a), "rotations": q / d[:, None], "opacities": self.sigmoid(x), "norm": n}
            if epsilon is not None:
                v = self.clamp(out["opacities"], epsilon)
                terms = self.log(v) + self.log(T(1) - v)
                out["terms"] = terms
                mean = terms.astype(D).sum() / D(terms.size)        # float32 terms, float64 sum and division, one rounding
                out["reg"] = T(mean)
        assert all(v.dtype == T for v in out.values())
        return out

    def activate_backward(self, rotation, scales, opacities, g_scales=None, g_rotations=None, g_opacities=None, g_reg=None, epsilon=1e-3):
        T = self.T
        q, s, o = self._a(rotation), self._a(scales), self._a(opacities).reshape(-1)
        N = q.shape[0]
        gs, gr, go = self._a(g_scales), self._a(g_rotations), self._a(g_opacities)
        with np.errstate(all="ignore"):
            d_scaling = np.zeros((N, 3), T) if gs is None else gs * s
            if gr is None:
                d_rotation = np.zeros((N, 4), T)
            else:
                n = self.norm(q)
                r = q / n[:, None]
                t = ((r[:, 0] * gr[:, 0] + r[:, 1] * gr[:, 1]) + r[:, 2] * gr[:, 2]) + r[:, 3] * gr[:, 3]
                above = (gr - r * t[:, None]) / n[:, None]
                d_rotation = np.where((n >= T(NORM_EPS))[:, None], above, gr / T(NORM_EPS))
            if go is None and g_reg is None:
                d_opacity = np.zeros(N, T)
            else:
                go = np.zeros(N, T) if go is None else go.reshape(-1)
                t = np.zeros(N, T)
                if g_reg is not None:
                    c = T(g_reg) / T(N)
                    e, hi = T(epsilon), T(1) - T(epsilon)
                    v = self.clamp(o, epsilon)
                    w = T(1) / v - T(1) / (T(1) - v)
                    t = np.where((e <= o) & (o <= hi), c * w, T(0))
                d_opacity = (go + t) * (o * (T(1) - o))
        assert d_scaling.dtype == d_rotation.dtype == d_opacity.dtype == T
        return d_scaling, d_rotation, d_opacity

    def _frame(self, scaling, rotation, modifier):
        T = self.T
        a, q = self._a(scaling), self._a(rotation)
        s = T(modifier) * self.exp(a)
        n = self.norm(q)
        qh = q / n[:, None]
        r, x, y, z = qh[:, 0], qh[:, 1], qh[:, 2], qh[:, 3]
        one, two = T(1), T(2)
        R = np.empty((q.shape[0], 3, 3), T)
        R[:, 0, 0] = one - two * (y * y + z * z)
        R[:, 0, 1] = two * (x * y - r * z)
        R[:, 0, 2] = two * (x * z + r * y)
        R[:, 1, 0] = two * (x * y + r * z)
        R[:, 1, 1] = one - two * (x * x + z * z)
        R[:, 1, 2] = two * (y * z - r * x)
        R[:, 2, 0] = two * (x * z - r * y)
        R[:, 2, 1] = two * (y * z + r * x)
        R[:, 2, 2] = one - two * (x * x + y * y)
        L = R * s[:, None, :]
        return s, n, qh, R, L

    def covariance(self, scaling, rotation, modifier=1.0):
        with np.errstate(all="ignore"):
            s, n, qh, R, L = self._frame(scaling, rotation, modifier)
            dot = lambda i, j: (L[:, i, 0] * L[:, j, 0] + L[:, i, 1] * L[:, j, 1]) + L[:, i, 2] * L[:, j, 2]
            cov = np.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], axis=1)
        assert cov.dtype == self.T
        return cov

    def covariance_backward(self, scaling, rotation, modifier, g_cov):
        T = self.T
        N = np.asarray(rotation).shape[0]
        if g_cov is None:
            return np.zeros((N, 3), T), np.zeros((N, 4), T)
        g = self._a(g_cov)
        two = T(2)
        with np.errstate(all="ignore"):
            s, n, qh, R, L = self._frame(scaling, rotation, modifier)
            M = [[two * g[:, 0], g[:, 1], g[:, 2]], [g[:, 1], two * g[:, 3], g[:, 4]], [g[:, 2], g[:, 4], two * g[:, 5]]]
            Dm = np.empty((N, 3, 3), T)
            da = np.empty((N, 3), T)
            for k in range(3):
                dL = [(M[i][0] * L[:, 0, k] + M[i][1] * L[:, 1, k]) + M[i][2] * L[:, 2, k] for i in range(3)]
                da[:, k] = ((dL[0] * R[:, 0, k] + dL[1] * R[:, 1, k]) + dL[2] * R[:, 2, k]) * s[:, k]
                for i in range(3):
                    Dm[:, i, k] = dL[i] * s[:, k]
            r, x, y, z = qh[:, 0], qh[:, 1], qh[:, 2], qh[:, 3]
            x2, y2, z2 = two * x, two * y, two * z
            d = lambda i, k: Dm[:, i, k]
            u = np.empty((N, 4), T)
            u[:, 0] = two * ((((((-z) * d(0, 1) + y * d(0, 2)) + z * d(1, 0)) - x * d(1, 2)) - y * d(2, 0)) + x * d(2, 1))
            u[:, 1] = two * (((((((y * d(0, 1) + z * d(0, 2)) + y * d(1, 0)) - x2 * d(1, 1)) - r * d(1, 2)) + z * d(2, 0)) + r * d(2, 1))
                             - x2 * d(2, 2))
            u[:, 2] = two * ((((((((-y2) * d(0, 0) + x * d(0, 1)) + r * d(0, 2)) + x * d(1, 0)) + z * d(1, 2)) - r * d(2, 0)) + z * d(2, 1))
                             - y2 * d(2, 2))
            u[:, 3] = two * ((((((((-z2) * d(0, 0) - r * d(0, 1)) + x * d(0, 2)) + r * d(1, 0)) - z2 * d(1, 1)) + y * d(1, 2)) + x * d(2, 0))
                             + y * d(2, 1))
            t = ((qh[:, 0] * u[:, 0] + qh[:, 1] * u[:, 1]) + qh[:, 2] * u[:, 2]) + qh[:, 3] * u[:, 3]
            dq = (u - qh * t[:, None]) / n[:, None]
        assert da.dtype == dq.dtype == T
        return da, dq


S64, S32 = Statement(D), Statement(F)


# ---- inputs shared by the host test, the GPU test and scripts/params_parity.py ----
def random_rows(N, seed):
    """Finite random parameters: scaling in [-12, 4], quaternions of norm 1e-3 .. 1e3 (log-uniform), logits in [-12, 12]"""
    rng = np.random.default_rng(seed)
    scaling = rng.uniform(-12.0, 4.0, (N, 3)).astype(F)
    q = rng.standard_normal((N, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3.0, 3.0, (N, 1))
    opacity = rng.uniform(-12.0, 12.0, (N, 1)).astype(F)
    return scaling, q.astype(F), opacity


def random_grads(N, seed):
    """Upstream gradients of order one, and the regulariser's"""
    rng = np.random.default_rng(seed + 1000)
    g = lambda *s: rng.standard_normal(s).astype(F)
    return {"g_scales": g(N, 3), "g_rotations": g(N, 4), "g_opacities": g(N, 1), "g_reg": F(rng.uniform(0.5, 2.0)), "g_cov": g(N, 6)}


def edge_logits(epsilon=1e-3):
    """The logits whose float32-statement sigmoid is nearest to the float32 epsilon and to 1 - epsilon, with their float32
    neighbours on both sides: for each edge the last logit below it, the first at or above it, the last at or below it and the
    first above it, each with its two neighbours (near 1 - epsilon many logits share one sigmoid; near epsilon a step of the logit
    moves the sigmoid by several units in the last place, so epsilon itself may not be reached -- `edge_opacities` covers that).
    Found by bisection on the statement."""
    out = []
    for target in (F(epsilon), F(1) - F(epsilon)):
        for below in (lambda o: o < target, lambda o: o <= target):         # the first logit at the edge, and the first one past it
            lo, hi = F(-20), F(20)
            while np.nextafter(lo, hi) < hi:
                mid = F((D(lo) + D(hi)) / 2)
                if below(S32.sigmoid(np.array([mid], F))[0]):
                    lo = mid
                else:
                    hi = mid
            for c in (lo, hi):
                out += [np.nextafter(c, F(-100)), c, np.nextafter(c, F(100))]
    return np.unique(np.array(out, F))


def edge_opacities(epsilon=1e-3):
    """The float32 epsilon and 1 - epsilon themselves with their neighbours, in ascending order: handed to the backward as saved
    opacities, they hit the clamp's inclusive edges exactly (no logit does)"""
    lo, hi = F(epsilon), F(1) - F(epsilon)
    return np.array([np.nextafter(lo, F(0)), lo, np.nextafter(lo, F(1)), np.nextafter(hi, F(0)), hi, np.nextafter(hi, F(1))], F)


def special_rows(epsilon=1e-3):
    """(scaling, rotation, opacity) of the rows the GPU test checks for class and bits"""
    quats = [[0, 0, 0, 0], [1e-25, 1e-25, 1e-25, 1e-25], [1e25, 1e25, 1e25, 1e25], [1e-25, 0, 0, 0], [0, -1e25, 3e24, 0],
             [1, 0, 0, 0], [0.5, -0.5, 0.5, -0.5], [3e-13, 0, 0, 0], [1e-12, 0, 0, 0], [0, 2e-12, 0, 0]]
    scal = [89.0, -104.0, 88.0, -103.0, 0.0, -87.0, 3.5, -110.5, 95.0, -20.0]
    logits = [17.0, -17.0, 90.0, -90.0, 0.0, -0.0, 88.0, -88.0, 104.0, -104.0] + edge_logits(epsilon).tolist()
    M = max(len(quats), len(scal), len(logits))
    rot = np.array([quats[i % len(quats)] for i in range(M)], F)
    sc = np.array([[scal[i % len(scal)], scal[(i + 1) % len(scal)], scal[(i + 2) % len(scal)]] for i in range(M)], F)
    op = np.array([logits[i % len(logits)] for i in range(M)], F).reshape(-1, 1)
    return sc, rot, op


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


def parity_fields(scaling, rotation, opacity, grads, epsilon=1e-3, modifier=1.0):
    """For finite rows: {field: (float64 truth, float32 statement, scale)} of every output of the stage, forward and backward, with
    the scales the parity bound is stated in: the element's own magnitude for scales, opacities and the gradients of scaling and
    opacity; 1 for the unit quaternion; the row's |g_r| / n for the gradient of rotation; the row's largest s^2 for the covariance
    and its gradients (the upstream gradients are of order one)."""
    out = {}
    fwd = {}
    for S in (S64, S32):
        f = S.activate(scaling, rotation, opacity, epsilon)
        b = S.activate_backward(rotation, f["scales"], f["opacities"], grads["g_scales"], grads["g_rotations"], grads["g_opacities"],
                                grads["g_reg"], epsilon)
        cov = S.covariance(scaling, rotation, modifier)
        cb = S.covariance_backward(scaling, rotation, modifier, grads["g_cov"])
        fwd[S.T] = dict(scales=f["scales"], rotations=f["rotations"], opacities=f["opacities"], reg=np.array([f["reg"]]), d_scaling=b[0],
                        d_rotation=b[1], d_opacity=b[2], cov=cov, cov_d_scaling=cb[0], cov_d_rotation=cb[1])
    t = fwd[D]
    n = S64.norm(np.asarray(rotation, D))
    gr = np.linalg.norm(np.asarray(grads["g_rotations"], D), axis=1)
    s2 = (modifier * np.exp(np.asarray(scaling, D))).max(axis=1) ** 2
    scale = dict(scales=np.abs(t["scales"]), rotations=1.0, opacities=np.abs(t["opacities"]), reg=np.abs(t["reg"]),
                 d_scaling=np.abs(t["d_scaling"]), d_rotation=(gr / n)[:, None], d_opacity=np.abs(t["d_opacity"]),
                 cov=s2[:, None], cov_d_scaling=s2[:, None], cov_d_rotation=s2[:, None])
    for k in t:
        out[k] = (t[k], fwd[F][k], scale[k])
    return out


PARITY_FACTOR = 4.0             # the project's standing bound (MLP, LPIPS, K1 / K8): 4 x the float32 statement's own error ...
PARITY_FLOOR = 2.0 ** -24       # ... which is itself floored at half a unit in the last place


def same_class_and_bits(a, b):
    """zero / infinity / NaN in the same places, and equal bits where finite (so the sign of a zero counts)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])
