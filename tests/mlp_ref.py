"""The float64 statement of the fused MLP (include/texgs_mlp.h, texgs/mlp.py) in numpy: forward, dx and d_params in the flat layout.

    pin = pad16(n_in), pout = pad16(n_out);  params = W_1 [128, pin] | L - 1 x [128, 128] | W_out [pout, 128], row-major
    xp  = [x | 1 ... 1];  h_1 = relu(W_1 xp);  h_k = relu(W_k h_{k-1});  y = (W_out h_L)[:n_out]
    backward: dy padded with zero columns to pout; dW_out = dyp^T h_L; d_L = (dyp W_out) . [h_L > 0]; ...; dW_1 = d_1^T xp;
              dx = (d_1 W_1)[:, :n_in]

`fp32=True` evaluates the same chain in float32 on the CPU (every matrix product and sum in float32): another fp32 evaluation, whose own
error against the float64 one sizes the GPU tests' tolerance.  A spec is (n_in, n_out, n_hidden_layers)."""
import numpy as np

WIDTH = 128


def pad16(k):
    return -(-int(k) // 16) * 16


def shapes(spec):
    n_in, n_out, L = spec
    return [(WIDTH, pad16(n_in))] + [(WIDTH, WIDTH)] * (L - 1) + [(pad16(n_out), WIDTH)]


def param_count(spec):
    return sum(a * b for a, b in shapes(spec))


def split(params, spec):
    """the matrices of a flat parameter vector, as views"""
    mats, off = [], 0
    for a, b in shapes(spec):
        mats.append(params[off:off + a * b].reshape(a, b))
        off += a * b
    assert off == params.shape[0]
    return mats


def xavier_params(spec, seed):
    """Xavier-uniform per matrix, float32"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, a * b) * np.sqrt(6.0 / (a + b)) for a, b in shapes(spec)]).astype(np.float32)


def _padded_input(x, spec, dt):
    n_in = spec[0]
    xp = np.ones((x.shape[0], pad16(n_in)), dt)
    xp[:, :n_in] = x
    return xp


def pre_activations(params, x, spec, fp32=False):
    """[z_1, ..., z_L]: the hidden layers' pre-activations"""
    dt = np.float32 if fp32 else np.float64
    mats = split(np.asarray(params).astype(dt), spec)
    h = _padded_input(np.asarray(x).astype(dt), spec, dt)
    zs = []
    for W in mats[:-1]:
        z = h @ W.T
        zs.append(z)
        h = np.maximum(z, 0)
    return zs


def forward(params, x, spec, fp32=False):
    dt = np.float32 if fp32 else np.float64
    mats = split(np.asarray(params).astype(dt), spec)
    h = _padded_input(np.asarray(x).astype(dt), spec, dt)
    for W in mats[:-1]:
        h = np.maximum(h @ W.T, 0)
    return (h @ mats[-1].T)[:, :spec[1]]


def backward(params, x, dy, spec, fp32=False):
    """(dx [N, n_in], d_params flat) for the upstream gradient dy [N, n_out]"""
    dt = np.float32 if fp32 else np.float64
    n_in, n_out, L = spec
    mats = split(np.asarray(params).astype(dt), spec)
    hs = [_padded_input(np.asarray(x).astype(dt), spec, dt)]
    for W in mats[:-1]:
        hs.append(np.maximum(hs[-1] @ W.T, 0))
    d = np.zeros((hs[0].shape[0], pad16(n_out)), dt)
    d[:, :n_out] = np.asarray(dy).astype(dt)
    grads = [None] * len(mats)
    for k in range(len(mats) - 1, -1, -1):
        grads[k] = d.T @ hs[k]
        d = d @ mats[k]
        if k > 0:
            d = d * (hs[k] > 0)
    return d[:, :n_in], np.concatenate([g.reshape(-1) for g in grads])


def kink_free_inputs(spec, N, seed, params=None):
    """(params f32, x f32 [N, n_in]): Xavier weights (or `params`) and the first N of 2 N candidates uniform in [-1, 1] whose every hidden
    pre-activation, in float64, satisfies |z| >= 1e-3 rms(z of that layer): no ReLU mask can differ between two evaluations whose
    pre-activations agree to fp32 accuracy, so no row ever needs excluding from a comparison."""
    if params is None:
        params = xavier_params(spec, seed)
    rng = np.random.default_rng(seed + 1000003)
    cand = rng.uniform(-1, 1, (2 * N, spec[0])).astype(np.float32)
    ok = np.ones(2 * N, bool)
    for z in pre_activations(params, cand, spec):
        ok &= (np.abs(z) >= 1e-3 * np.sqrt(np.mean(z * z))).all(axis=1)
    keep = np.flatnonzero(ok)[:N]
    assert keep.size == N, f"kink_free_inputs: only {int(ok.sum())} of {2 * N} candidates are clear of every kink for {spec}"
    return params, np.ascontiguousarray(cand[keep])


def tolerance(f64, cpu_f32):
    """4 x max(the float32 CPU evaluation's own error, 2^-23 of the tensor's scale)"""
    f64 = np.asarray(f64, np.float64)
    return 4.0 * max(float(np.abs(np.asarray(cpu_f32, np.float64) - f64).max()) if f64.size else 0.0,
                     2.0 ** -23 * (float(np.abs(f64).max()) if f64.size else 0.0))
