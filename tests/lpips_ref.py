"""The float64 statement of LPIPS-VGG that the tests compare csrc/lpips.hip against: plain numpy, written from the definition in
include/texgs_lpips.h and texgs/lpips.py's docstring, independent of torch's convolution and of the code under test.

Every function takes `fp32=False`; with fp32=True the SAME loops run in float32 arrays in the same order -- for the convolution a plain
k-ordered fp32 chain, one (input channel, tap) product plane at a time -- which is the yardstick of `tolerance`: a bound on another
fp32 evaluation comes from this fp32 evaluation's own error, never from the code under test."""
import numpy as np

SLICES = (2, 2, 3, 3, 3)                      # convolutions per slice; a 2x2 max-pool stands in front of slices 2-5
SHIFT = (-0.030, -0.088, -0.188)              # the scaling layer of lpips 0.1: (x - shift) / scale
SCALE = (0.458, 0.448, 0.450)


def maxpool2(x):
    """2x2 / stride 2 / floor mode over the last two axes: an odd last row or column is dropped"""
    H, W = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., :2 * H, :2 * W]
    return np.maximum(np.maximum(x[..., 0::2, 0::2], x[..., 0::2, 1::2]), np.maximum(x[..., 1::2, 0::2], x[..., 1::2, 1::2]))


def conv3x3(x, w, b, relu=True, pool_in=False, in_scale=None, in_shift=None, fp32=False):
    """y [B,Cout,Ho,Wo] = act(conv3x3(pad1(in(x))) + b): x [B,Cin,H,W], w [Cout,Cin,3,3], stride 1, zero padding 1.
    in(x) = x * in_scale + in_shift per channel (when given), then the 2x2 max-pool (with pool_in); the padding zeros live behind
    both.  The sum runs over (input channel, tap) in that order, one product plane at a time."""
    dt = np.float32 if fp32 else np.float64
    x, w, b = np.asarray(x, dt), np.asarray(w, dt), np.asarray(b, dt)
    if in_scale is not None:
        x = x * np.asarray(in_scale, dt)[None, :, None, None] + np.asarray(in_shift, dt)[None, :, None, None]
    if pool_in:
        x = maxpool2(x)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xp = np.zeros((B, Cin, H + 2, W + 2), dt)
    xp[:, :, 1:-1, 1:-1] = x
    acc = np.zeros((B, Cout, H, W), dt)
    for ci in range(Cin):
        for dy in range(3):
            for dx in range(3):
                acc += w[None, :, ci, dy, dx, None, None] * xp[:, None, ci, dy:dy + H, dx:dx + W]
    acc += b[None, :, None, None]
    if relu:
        acc = np.maximum(acc, dt(0))
    assert acc.dtype == dt
    return acc


def input_affine(normalize, dt=np.float32):
    """(in_scale, in_shift) of the first convolution as float32 -- the values the device gets: ((2x - 1) - shift) / scale with
    `normalize`, (x - shift) / scale without"""
    shift, scale = np.asarray(SHIFT, np.float64), np.asarray(SCALE, np.float64)
    if normalize:
        return (2.0 / scale).astype(dt), ((-1.0 - shift) / scale).astype(dt)
    return (1.0 / scale).astype(dt), (-shift / scale).astype(dt)


def features(convs, x, normalize=False, fp32=False):
    """The five tapped maps of x [B,3,H,W]; convs = thirteen (w, b) pairs"""
    sc, sh = input_affine(normalize)
    taps, k, h = [], 0, x
    for s, n in enumerate(SLICES):
        for j in range(n):
            w, b = convs[k]
            h = conv3x3(h, w, b, True, s > 0 and j == 0, sc if k == 0 else None, sh if k == 0 else None, fp32)
            k += 1
        taps.append(h)
    return taps


def head(f0, f1, lin, fp32=False):
    """One layer's term per pair: f0, f1 [P,C,h,w], lin [C] -> float64 [P].  Per pixel in the working precision, sums over channels
    in channel order: n = sqrt(sum f^2), d = sum lin (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10))^2; over pixels in float64."""
    dt = np.float32 if fp32 else np.float64
    f0, f1, lin = np.asarray(f0, dt), np.asarray(f1, dt), np.asarray(lin, dt)
    P, C, h, w = f0.shape
    q0, q1 = np.zeros((P, h, w), dt), np.zeros((P, h, w), dt)
    for c in range(C):
        q0 += f0[:, c] * f0[:, c]
        q1 += f1[:, c] * f1[:, c]
    n0, n1 = np.sqrt(q0) + dt(1e-10), np.sqrt(q1) + dt(1e-10)
    d = np.zeros((P, h, w), dt)
    for c in range(C):
        e = f0[:, c] / n0 - f1[:, c] / n1
        d += lin[c] * (e * e)
    assert d.dtype == dt
    return d.astype(np.float64).sum(axis=(1, 2)) / float(h * w)


def layers(convs, lins, img0, img1, normalize=False, fp32=False):
    """float64 [P,5]: the five layers' terms of the pairs img0 / img1 [P,3,H,W]"""
    P = img0.shape[0]
    taps = features(convs, np.concatenate([img0, img1]), normalize, fp32)
    return np.stack([head(t[:P], t[P:], lin, fp32) for t, lin in zip(taps, lins)], axis=1)


def lpips(convs, lins, img0, img1, normalize=False, fp32=False):
    """float64 [P]: the sum of the five terms, added in layer order"""
    L = layers(convs, lins, img0, img1, normalize, fp32)
    v = L[:, 0].copy()
    for k in range(1, 5):
        v = v + L[:, k]
    return v


def tolerance(f64, f32):
    """4 x max(the float32 statement's own error, 2^-23 of the tensor's scale): the rule of mlp_ref.tolerance"""
    f64 = np.asarray(f64, np.float64)
    return 4.0 * max(float(np.abs(np.asarray(f32, np.float64) - f64).max()) if f64.size else 0.0,
                     2.0 ** -23 * (float(np.abs(f64).max()) if f64.size else 0.0))
