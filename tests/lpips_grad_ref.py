"""The float64 statement of the backward of LPIPS-VGG in the images that the tests compare csrc/lpips_grad.hip and the chain of
texgs/lpips.py against: plain numpy, written from include/texgs_lpips_grad.h, independent of torch's autograd and of the code under
test.  Three pieces -- the head's backward, the unpool + gate that finishes a tapped layer, the transposed convolution -- and the whole
chain GIVEN THE THIRTEEN ACTIVATION MAPS.

Taking the maps as an input is the point: ReLU masks and pool arg-maxes are discrete, a float32 and a float64 forward can disagree on
them, and then no tolerance means anything.  Given the same stored maps the backward is a continuous function with no decision left
to take, so no element is excluded anywhere.

Every function takes `fp32=False`; with fp32=True the SAME loops run in float32 arrays in the same order, as in tests/lpips_ref.py:
that evaluation's own error is the yardstick of lpips_ref.tolerance."""
import numpy as np

import lpips_ref as R

SLICES = R.SLICES


def forward_maps(convs, x, normalize=False, fp32=False):
    """The thirteen post-ReLU maps of x [B,3,H,W] (lpips_ref.features keeps five of them); convs = thirteen (w, b) pairs"""
    sc, sh = R.input_affine(normalize)
    maps, k, h = [], 0, x
    for s, n in enumerate(SLICES):
        for j in range(n):
            w, b = convs[k]
            h = R.conv3x3(h, w, b, True, s > 0 and j == 0, sc if k == 0 else None, sh if k == 0 else None, fp32)
            maps.append(h)
            k += 1
    return maps


def head_backward(f0, f1, lin, gbar, fp32=False):
    """The gradient of sum_p gbar_p head_p (lpips_ref.head) in f0 and f1 [P,C,h,w] -> (h0, h1).  Per pixel, sums over channels in
    channel order:  n = sqrt(sum f^2), d = n + 1e-10, r_c = (2 lin_c) (f0_c / d0 - f1_c / d1), t0 = sum r_c f0_c, t1 = sum r_c f1_c,
    s = gbar_p / (h w);  h0_c = s (r_c / d0 - f0_c (t0 / (n0 d0^2))),  h1_c = s (-r_c / d1 - f1_c (-t1 / (n1 d1^2))).
    A pixel whose n is 0 gets a zero row (the rule of texgs_lpips_grad.h: the derivative of sqrt at 0 is not finite)."""
    dt = np.float32 if fp32 else np.float64
    f0, f1, lin, gbar = np.asarray(f0, dt), np.asarray(f1, dt), np.asarray(lin, dt), np.asarray(gbar, dt)
    P, C, h, w = f0.shape
    q0, q1 = np.zeros((P, h, w), dt), np.zeros((P, h, w), dt)
    for c in range(C):
        q0 += f0[:, c] * f0[:, c]
        q1 += f1[:, c] * f1[:, c]
    n0, n1 = np.sqrt(q0), np.sqrt(q1)
    d0, d1 = n0 + dt(1e-10), n1 + dt(1e-10)
    t0, t1 = np.zeros((P, h, w), dt), np.zeros((P, h, w), dt)
    r = np.zeros((P, C, h, w), dt)
    for c in range(C):
        r[:, c] = (dt(2) * lin[c]) * (f0[:, c] / d0 - f1[:, c] / d1)
        t0 += r[:, c] * f0[:, c]
        t1 += r[:, c] * f1[:, c]
    s = (gbar / dt(h * w))[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        k0, k1 = t0 / (n0 * (d0 * d0)), (-t1) / (n1 * (d1 * d1))
        h0 = np.where((n0 > 0)[:, None], s[:, None] * (r / d0[:, None] - f0 * k0[:, None]), dt(0))
        h1 = np.where((n1 > 0)[:, None], s[:, None] * ((-r) / d1[:, None] - f1 * k1[:, None]), dt(0))
    assert h0.dtype == dt and h1.dtype == dt
    return h0, h1


def first_max(f):
    """Per 2x2 / stride-2 window of the last two axes of f: the position (0..3, row-major) of its FIRST maximum -> int [..., h//2, w//2]"""
    H, W = f.shape[-2] // 2, f.shape[-1] // 2
    v = f[..., :2 * H, :2 * W]
    v00, v01, v10, v11 = v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]
    m = np.maximum(np.maximum(v00, v01), np.maximum(v10, v11))
    return np.where(v00 == m, 0, np.where(v01 == m, 1, np.where(v10 == m, 2, 3)))


def unpool(f, g_next):
    """The backward of the 2x2 max-pool of f [...,h,w]: g_next [...,h//2,w//2] goes to the first maximum of each window; every
    other pixel -- the odd last row and column too -- gets 0"""
    H, W = f.shape[-2] // 2, f.shape[-1] // 2
    first = first_max(f)
    out = np.zeros(f.shape, g_next.dtype)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[..., dy:2 * H:2, dx:2 * W:2] = np.where(first == k, g_next, g_next.dtype.type(0))
    return out


def finish(f, head, g_next=None, fp32=False):
    """G = f > 0 ? unpool(g_next) + head : 0 -- what texgs_lpips_head_backward stores for a tapped map f"""
    dt = np.float32 if fp32 else np.float64
    f, g = np.asarray(f, dt), np.asarray(head, dt)
    if g_next is not None:
        g = unpool(f, np.asarray(g_next, dt)) + g
    return np.where(f > 0, g, dt(0))


def gate(g, y, fp32=False):
    dt = np.float32 if fp32 else np.float64
    return np.where(np.asarray(y) > 0, np.asarray(g, dt), dt(0))


def conv3x3_transposed(g, w, fp32=False):
    """The data gradient of y = conv3x3(pad1(x), w) (stride 1, zero padding 1): g [B,Cout,H,W] = dL/dy, w [Cout,Cin,3,3] ->
    dL/dx [B,Cin,H,W], from the definition: x[ci, y + dy - 1, x + dx - 1] feeds y[co, y, x] with weight w[co, ci, dy, dx], so
    dL/dx[ci, u, v] = sum_co sum_dy sum_dx w[co, ci, dy, dx] g[co, u - dy + 1, v - dx + 1] with g zero outside the image.  The sum
    runs over (co, tap) with the taps last first, one product plane at a time."""
    dt = np.float32 if fp32 else np.float64
    g, w = np.asarray(g, dt), np.asarray(w, dt)
    B, Cout, H, W = g.shape
    Cin = w.shape[1]
    gp = np.zeros((B, Cout, H + 2, W + 2), dt)
    gp[:, :, 1:-1, 1:-1] = g
    acc = np.zeros((B, Cin, H, W), dt)
    for co in range(Cout):
        for dy in (2, 1, 0):
            for dx in (2, 1, 0):          # g[u - dy + 1] = gp[u - dy + 2]
                acc += w[co, :, dy, dx][None, :, None, None] * gp[:, None, co, 2 - dy:2 - dy + H, 2 - dx:2 - dx + W]
    assert acc.dtype == dt
    return acc


def backward(convs, lins, maps, gbar, normalize=False, fp32=False):
    """The gradient of sum_p gbar_p lpips_p in the 2P images, GIVEN the thirteen post-ReLU maps [2P, C, h, w] of a forward (first
    images, then their partners) -> [2P,3,H,W] in the working precision.  No decision is taken here that the maps do not fix."""
    dt = np.float32 if fp32 else np.float64
    P = maps[0].shape[0] // 2
    k, g_next = len(maps) - 1, None
    for s in reversed(range(len(SLICES))):
        tap = np.asarray(maps[k], dt)
        h0, h1 = head_backward(tap[:P], tap[P:], lins[s], gbar, fp32)
        grad = finish(tap, np.concatenate([h0, h1]), g_next, fp32)
        for j in reversed(range(SLICES[s])):
            gin = conv3x3_transposed(grad, convs[k][0], fp32)
            if j > 0:
                grad = gate(gin, maps[k - 1], fp32)
            else:
                g_next = gin
            k -= 1
    out = g_next * np.asarray(R.input_affine(normalize)[0], dt)[None, :, None, None]
    assert out.dtype == dt
    return out
