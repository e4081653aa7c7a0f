"""The statement of the fused Adam step (csrc/optim.hip, texgs/optim.py) in numpy float32: one astype(float32) per operation, in the
order of the contract, scalars prepared exactly as texgs.optim.scalars prepares them.  The GPU tests compare with it bit for bit;
tests/test_optim_host.py compares IT with torch's CPU Adam in scaled units."""
import ctypes

import numpy as np

F = np.float32
TINY = float(np.finfo(np.float32).tiny)         # smallest normal f32: the floor of every scale below
UNIT = 2.0 ** -24


def f32(x):
    return ctypes.c_float(x).value


def scalars(step, lr, betas, eps):
    """(w1, beta2, w2, bc2_sqrt, eps, neg_step_size), Python doubles rounded to f32 once (texgs.optim.scalars)"""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step, lr = float(step), float(lr)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    return tuple(F(f32(x)) for x in (1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, float(eps), -step_size))


def adam_np(p, g, m, v, step, lr, betas, eps):
    """One step of one tensor with the counter ALREADY advanced to `step`: -> (p', m', v') as new float32 arrays"""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    w1, beta2, w2, bc2_sqrt, eps, neg_step_size = scalars(step, lr, betas, eps)
    with np.errstate(all="ignore"):
        d = (g - m).astype(F)
        if w1 < F(0.5):
            m1 = (m + (w1 * d).astype(F)).astype(F)
        else:
            one_minus_w1 = F(F(1.0) - w1)
            m1 = (g - (d * one_minus_w1).astype(F)).astype(F)
        v1 = (v * beta2).astype(F)
        v1 = (v1 + ((w2 * g).astype(F) * g).astype(F)).astype(F)
        den = ((np.sqrt(v1).astype(F) / bc2_sqrt).astype(F) + eps).astype(F)
        p1 = (p + (neg_step_size * (m1 / den).astype(F)).astype(F)).astype(F)
    return p1, m1, v1


def step_np(tensors):
    """tensors: list of (p, g, m, v, step, lr, betas, eps) with `step` the counter BEFORE the call -> list of (p', m', v', step + 1)"""
    out = []
    for p, g, m, v, step, lr, betas, eps in tensors:
        p1, m1, v1 = adam_np(p, g, m, v, step + 1, lr, betas, eps)
        out.append((p1, m1, v1, step + 1))
    return out


def same_bits(a, b):
    """float32 arrays equal as bit patterns, NaNs compared by position"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def scaled_units(p0, g, m0, v0, got, want):
    """The largest differences of (p', m', v') `got` from `want` in units of 2^-24 of a scale: m' against max(|m|, |g|), v' against
    max(v, g^2), p' against max(|p|, |p' - p|) (the reference's p'), each floored at the smallest normal f32.  Plain ulps of the
    output mean nothing under the lerp's cancellation.  -> (units_p, units_m, units_v) in float64"""
    p0, g, m0, v0 = (np.asarray(a, np.float64) for a in (p0, g, m0, v0))
    gp, gm, gv = (np.asarray(a, np.float64) for a in got)
    wp, wm, wv = (np.asarray(a, np.float64) for a in want)
    sm = np.maximum(np.maximum(np.abs(m0), np.abs(g)), TINY)
    sv = np.maximum(np.maximum(v0, g * g), TINY)
    sp = np.maximum(np.maximum(np.abs(p0), np.abs(wp - p0)), TINY)
    u = lambda a, b, s: float((np.abs(a - b) / (s * UNIT)).max())
    return u(gp, wp, sp), u(gm, wm, sm), u(gv, wv, sv)


def parity_inputs(n=65536, seed=0):
    """The inputs of the comparisons with torch's own Adam: gradient magnitudes log-uniform in 1e-24 .. 1e2 with random signs, every
    7th gradient 0; parameters of order 1.  -> (p f32[n], grads: callable k -> f32[n] of step k)"""
    rng = np.random.RandomState(seed)
    p = rng.randn(n).astype(F)

    def grad(k):
        r = np.random.RandomState(seed * 1000 + 17 + k)
        mag = 10.0 ** r.uniform(-24.0, 2.0, n)
        g = (mag * r.choice([-1.0, 1.0], n)).astype(F)
        g[::7] = 0.0
        return g
    return p, grad
