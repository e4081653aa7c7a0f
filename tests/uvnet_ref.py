"""The statement the UV-net kernels of csrc/uvnet.hip are tested against, row by row and entry by entry: plain torch on the CPU.

`forward` is the network with its Jacobian in forward mode, as the kernel propagates it (one value column and three tangent columns,
ReLU masks from the value column, bias first and then the embedding on layer 2, F.normalize with its 1e-12 clamp), in float64 or
float32, with the split-bf16 product of the kernels on the planes a precision runs that way.  `backward` is the chain behind
`texgs_uv_backward`, with -- in float64 -- the SCALE of every output entry: the sum over points of the absolute values of the terms
the entry sums, the unit its error is measured in.

Probe networks make the kernels' matrix products exact: every operand has few enough bits that a product, every partial sum of a row
in any order, and the split x = bf16(x) + bf16(x - bf16(x)) lose nothing, so a mis-packed weight, a wrong k-assignment or a missing
hi.lo step changes an exact number by order one in a named row.  `safe_points` chooses inputs of a random net away from ReLU kinks
(a choice of INPUTS: no output row is ever left out of a comparison)."""
import functools
import os

import numpy as np
import torch

HIDDEN = 128
FLOOR = 2.0 ** -24
BAR = 4.0                         # device error <= BAR x max(float32 statement's error, FLOOR)
SPLIT_PLANES = {"fp32": (), "mixed": (1, 2, 3), "bf16x3": (0, 1, 2, 3)}
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5")
SHAPES = {"W1": (HIDDEN, 3), "W5": (3, HIDDEN), "b5": (3,), **{f"W{k}": (HIDDEN, HIDDEN) for k in (2, 3, 4)},
          **{f"b{k}": (HIDDEN,) for k in (1, 2, 3, 4)}}


class Net:
    """W[0..4], b[0..4] (a bias may be None = the C ABI's NULL pointer), xyz_offset / xyz_scale (both or neither); float64 tensors
    holding float32 values."""

    def __init__(self, W, b, off=None, scale=None):
        self.W = [w.detach().double().contiguous() for w in W]
        self.b = [None if x is None else x.detach().double().contiguous() for x in b]
        self.off = None if off is None else torch.as_tensor(off).double()
        self.scale = None if scale is None else torch.as_tensor(scale).double()

    def without_bias(self):
        return Net(self.W, [None] * 5, self.off, self.scale)

    def with_zero_bias(self):
        return Net(self.W, [torch.zeros(w.shape[0]) for w in self.W], self.off, self.scale)

    def without_norm(self):
        return Net(self.W, self.b)

    def with_unit_norm(self):
        return Net(self.W, self.b, torch.zeros(3), torch.ones(3))


def from_module(m):
    lins = m._linears()
    both = m.xyz_offset is not None and m.xyz_scale is not None
    return Net([l.weight for l in lins], [l.bias for l in lins], m.xyz_offset if both else None, m.xyz_scale if both else None)


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def split_bf16(x):
    """x (any float dtype, float32 values) -> (hi, lo) as float32: hi = bf16(x), lo = bf16(x - hi), round to nearest even both."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def rejoin(x):
    hi, lo = split_bf16(x)
    return (hi + lo).to(x.dtype)


def product(X, W, split=False):
    """X [n, k] times W [m, k] transposed.  split: both operands as two bf16 halves, hi.hi + hi.lo + lo.hi accumulated in X's dtype,
    the lo.lo term dropped -- three matrix-core products per float32 product."""
    if not split:
        return X @ W.t()
    xh, xl = (t.to(X.dtype) for t in split_bf16(X))
    wh, wl = (t.to(X.dtype) for t in split_bf16(W))
    return xh @ wh.t() + xh @ wl.t() + xl @ wh.t()


def _norm_in(net, xyz, dtype):
    x = xyz.to(dtype)
    if net.off is None or net.scale is None:
        return x, torch.ones(3, dtype=dtype)
    inv = 1.0 / net.scale.to(dtype)
    return (x - net.off.to(dtype)) * inv, inv


def _layer1(net, xn, dtype):
    W1 = net.W[0].to(dtype)
    z = torch.zeros(xn.shape[0], HIDDEN, dtype=dtype) if net.b[0] is None else net.b[0].to(dtype)[None, :].expand(xn.shape[0], HIDDEN)
    for c in range(3):                                    # ((b + w0 x0) + w1 x1) + w2 x2, the kernels' order
        z = z + xn[:, c:c + 1] * W1[None, :, c]
    return z


def _pre(y, bias, emb, dtype):
    if bias is not None:
        y = y + bias.to(dtype)
    return y if emb is None else y + emb.to(dtype)


def sums(net, emb, xyz, dtype, split_planes=()):
    """-> o [N,3], dO [N,3,3] (dO[n,i,j] = d o_i / d x_j) and the four layers' pre-activations of the value column."""
    xn, inv = _norm_in(net, xyz, dtype)
    z = _layer1(net, xn, dtype)
    pres = [z]
    live = z > 0
    W1 = net.W[0].to(dtype)
    planes = [torch.where(live, z, torch.zeros_like(z))]
    planes += [torch.where(live, (W1[:, j] * inv[j])[None, :].expand_as(z), torch.zeros_like(z)) for j in range(3)]
    for k in (1, 2, 3):
        W = net.W[k].to(dtype)
        ys = [product(planes[t], W, t in split_planes) for t in range(4)]
        z = _pre(ys[0], net.b[k], emb if k == 1 else None, dtype)
        pres.append(z)
        live = z > 0
        planes = [torch.where(live, z, torch.zeros_like(z))] + [torch.where(live, ys[t], torch.zeros_like(z)) for t in (1, 2, 3)]
    W5 = net.W[4].to(dtype)
    outs = [(rejoin(planes[t]) if t in split_planes else planes[t]) @ W5.t() for t in range(4)]       # the output layer is float32 on the re-joined halves
    o = outs[0] if net.b[4] is None else outs[0] + net.b[4].to(dtype)
    return o, torch.stack(outs[1:], dim=2), pres


def finish(o, dO, dtype):
    """F.normalize and its Jacobian: uvs [N,3], J [N,9] with [3 i + j] = d uv_i / d x_j = ((I - u u^T) dO / |o|)[i, j]."""
    o, dO = o.to(dtype), dO.to(dtype)
    n = o.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    u = o / n
    ud = (u[:, :, None] * dO).sum(dim=1)                                   # [N, j]
    J = (dO - u[:, :, None] * ud[:, None, :]) / n[:, :, None]
    return u, J.reshape(-1, 9)


def finish_kernel_order(o, dO):
    """The normalise step in float32 in the kernel's own operation order (csrc/uvnet.hip uv_finish: 1 / |o| formed once and multiplied,
    fused multiply-adds where it has them, each sum of three products in its own order), so that on exact o / dO the kernel's BITS can
    be stated: torch's division-based `finish` is the same mathematics and other roundings.  A fused multiply-add is the float64 sum of
    the exact float64 product rounded to float32 (the float64 rounding in between can differ from the fused one only where the sum is
    within 2^-53 relative of a float32 tie); sqrt, division and multiplication are correctly rounded on both sides."""
    f = np.float32
    o, d = np.asarray(o, dtype=np.float64).astype(f), np.asarray(dO, dtype=np.float64).astype(f)          # d[n, i, j]
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    o0, o1, o2 = o[:, 0], o[:, 1], o[:, 2]
    rn = f(1.0) / np.maximum(np.sqrt(fma(o1, o1, o0 * o0) + o2 * o2), f(1e-12))
    u = [o0 * rn, o1 * rn, o2 * rn]
    ud = [fma(u[2], d[:, 2, 0], fma(u[0], d[:, 0, 0], u[1] * d[:, 1, 0])),
          fma(u[2], d[:, 2, 1], fma(u[1], d[:, 1, 1], u[0] * d[:, 0, 1])),
          fma(u[2], d[:, 2, 2], u[0] * d[:, 0, 2] + u[1] * d[:, 1, 2])]
    J = np.stack([fma(-u[i], ud[j], d[:, i, j]) * rn for i in range(3) for j in range(3)], axis=1)
    return torch.from_numpy(np.stack(u, axis=1)), torch.from_numpy(J)


def forward(net, emb, xyz, dtype, split_planes=()):
    o, dO, _ = sums(net, emb, xyz, dtype, split_planes)
    return finish(o, dO, dtype)


def backward(net, emb, xyz, g, dtype, split=False, scales=False):
    """The ten gradients of sum(uvs * g) as {name: tensor} (d emb = b2's).  split: the six products of the backward chain (W^T d and
    d h^T of the three 128 x 128 layers) as split-bf16 products; the recomputed forward, the thin layers and the sums stay in `dtype`.
    scales=True also returns {name: S}: per entry the sum over points of |term|."""
    xn, _ = _norm_in(net, xyz, dtype)
    W = [w.to(dtype) for w in net.W]
    z1 = _layer1(net, xn, dtype); h1 = z1.clamp_min(0)
    z2 = _pre(h1 @ W[1].t(), net.b[1], emb, dtype); a = z2.clamp_min(0)
    z3 = _pre(a @ W[2].t(), net.b[2], None, dtype); h2 = z3.clamp_min(0)
    z4 = _pre(h2 @ W[3].t(), net.b[3], None, dtype); h3 = z4.clamp_min(0)
    o = _pre(h3 @ W[4].t(), net.b[4], None, dtype)
    n = o.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    u = o / n
    gg = g.to(dtype)
    do = (gg - u * (u * gg).sum(dim=1, keepdim=True)) / n
    d4 = (do @ W[4]) * (z4 > 0)
    d3 = product(d4, W[3].t().contiguous(), split) * (z3 > 0)
    d2 = product(d3, W[2].t().contiguous(), split) * (z2 > 0)
    d1 = product(d2, W[1].t().contiguous(), split) * (z1 > 0)
    pairs = {"1": (d1, xn, False), "2": (d2, h1, split), "3": (d3, a, split), "4": (d4, h2, split), "5": (do, h3, False)}
    out = {}
    for k, (d, h, sp) in pairs.items():
        out["W" + k] = product(d.t().contiguous(), h.t().contiguous(), sp)
        out["b" + k] = d.sum(dim=0)
    if not scales:
        return out
    # The terms an entry sums, in absolute value.  A term is d[p, i] h[p, k], and both factors are themselves sums: d down the chain
    # from do = (g - u (u . g)) / |o| through W^T, h up from x through W.  Where such a sum cancels, its value says nothing about the
    # size of what was added to form it, and one rounding of the LARGEST addend is many units of the value for ANY float32 evaluation
    # (measured on the CPU, tests/test_uvnet_rows_host.py: with |d|^T |h| as the scale two float32 evaluations of the same chain in
    # two summation orders are 1e-3 of an entry's scale from float64 and a factor 12 from each other).  So the scale carries each
    # factor's own addends in absolute value -- m_k = (|d_{k+1}| |W_{k+1}|) . [z_k > 0] for d_k, a_k = (|W_k| |h_{k-1}| + |b_k| (+ |emb|)) .
    # [z_k > 0] for h_k, a_0 = (|x| + |offset|) / |scale| for the input, m_5 = c (|g| + |u| (|u| . |g|)) / |o| for do -- instead of |d| and
    # |h|:  S = m^T a for a weight, the column sum of m for a bias.  m >= |d| and a >= |h|, with equality where nothing cancels, and zero
    # exactly where the ReLU masks make the entry a sum of nothing.
    # The addends a sum received are themselves uncertain by THEIR scales, not by their values: where d_{k+1} is the small remainder of
    # a cancellation, |d_{k+1}| |W| is small too, yet d_k inherits d_{k+1}'s rounding error through W.  So each level also carries the
    # scales of the level it reads, through the same weights -- in quadrature, as independent roundings of different sums add:
    # m_k = sqrt((|d_{k+1}| |W|)^2 + m_{k+1}^2 W^2), a_k likewise from a_{k-1}.  (Carried linearly, |W| m_{k+1}, the scale is the
    # worst-case bound with every sign aligned: 1000 x above what any evaluation of a 128-wide net shows, and blind to a dropped point.)
    ab = lambda t: 0.0 if t is None else t.to(dtype).abs()
    live = lambda own, up, Wm, z: (own.pow(2) + up.pow(2) @ Wm.pow(2)).sqrt() * (z > 0)
    inv = torch.ones(3, dtype=dtype) if net.scale is None or net.off is None else 1.0 / net.scale.to(dtype).abs()
    a0 = (xyz.to(dtype).abs() + (0.0 if net.off is None or net.scale is None else net.off.to(dtype).abs())) * inv
    a1 = (a0 @ W[0].abs().t() + ab(net.b[0])) * (z1 > 0)
    a2 = live(h1 @ W[1].abs().t() + ab(net.b[1]) + ab(emb), a1, W[1].t(), z2)
    a3 = live(a @ W[2].abs().t() + ab(net.b[2]), a2, W[2].t(), z3)
    a4 = live(h2 @ W[3].abs().t() + ab(net.b[3]), a3, W[3].t(), z4)
    # (o is a cancelling sum too: its scale over its length, c >= 1, is how many roundings of |o| the direction u and 1 / |o| carry)
    a5 = live(h3 @ W[4].abs().t() + ab(net.b[4]), a4, W[4].t(), torch.ones_like(o))
    c = (a5.sum(dim=1, keepdim=True) / n).clamp_min(1.0)
    m5 = c * (gg.abs() + u.abs() * (u.abs() * gg.abs()).sum(dim=1, keepdim=True)) / n
    m4 = live(do.abs() @ W[4].abs(), m5, W[4], z4)
    m3 = live(d4.abs() @ W[3].abs(), m4, W[3], z3)
    m2 = live(d3.abs() @ W[2].abs(), m3, W[2], z2)
    m1 = live(d2.abs() @ W[1].abs(), m2, W[1], z1)
    S, S_plain = {}, {}
    for k, m, am in (("1", m1, a0), ("2", m2, a1), ("3", m3, a2), ("4", m4, a3), ("5", m5, a4)):
        d, h, _ = pairs[k]
        S["W" + k], S["b" + k] = m.t() @ am, m.sum(dim=0)
        S_plain["W" + k], S_plain["b" + k] = d.abs().t() @ h.abs(), d.abs().sum(dim=0)         # the sum of |term| with the factors as they are
    return out, S, S_plain


def reordered(net, emb, seed=0):
    """(Net, emb, permutations) of the same function with the hidden neurons of every layer permuted: the same sums in another order.
    The float32 statement's error is one draw per summation order; the yardstick of a bar is the larger of two."""
    gen = torch.Generator().manual_seed(seed)
    W, b, e = [w.clone() for w in net.W], [None if x is None else x.clone() for x in net.b], emb.clone()
    perms = [torch.randperm(HIDDEN, generator=gen) for _ in range(4)]
    for k, p in enumerate(perms):
        W[k] = W[k][p]
        b[k] = None if b[k] is None else b[k][p]
        e = e[p] if k == 1 else e
        W[k + 1] = W[k + 1][:, p]
    return Net(W, b, net.off, net.scale), e, perms


def backward_reordered(net, emb, xyz, g, dtype, split=False, seed=0):
    """backward() through reordered(), mapped back to the net's own neuron order."""
    net2, e, perms = reordered(net, emb, seed)
    out = backward(net2, e, xyz, g, dtype, split)
    for k, p in enumerate(perms):
        back = torch.argsort(p)
        out[f"W{k + 1}"], out[f"b{k + 1}"], out[f"W{k + 2}"] = out[f"W{k + 1}"][back], out[f"b{k + 1}"][back], out[f"W{k + 2}"][:, back]
    return out


# ------------------------------------------------------------------------------------------------------------------ errors
def row_error(got, ref):
    """Per row: max |got - ref| over the row / max |ref| of the row."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1e-300)


def entry_error(got, ref, S):
    """Largest |got - ref| / S over the entries; an entry whose scale is zero sums nothing but zeros and must be exactly the reference."""
    d = (got.double() - ref.double()).abs().reshape(-1)
    s = S.double().reshape(-1)
    e = torch.where(s > 0, d / s.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def worst_entry(got, ref, S):
    d = (got.double() - ref.double()).abs() / S.double().clamp_min(1e-300)
    i = int(d.reshape(-1).argmax())
    return tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))


def same_bits(a, b):
    return torch.equal(a.float().contiguous().view(torch.int32), b.float().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ probe networks
PROBE_OFFSET, PROBE_SCALE = (1.0, -2.0, 3.0), (2.0, 0.5, 4.0)        # integer offset, power-of-two scale
PROBE_KINDS = ("A", "B2", "B3", "B4")


def _sparse(gen, values, lo, hi):
    W = torch.zeros(HIDDEN, HIDDEN, dtype=torch.float64)
    for i in range(HIDDEN):
        nz = int(torch.randint(lo, hi + 1, (1,), generator=gen))
        cols = torch.randperm(HIDDEN, generator=gen)[:nz]
        W[i, cols] = values[torch.randint(0, len(values), (nz,), generator=gen)]
    return W


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def probe(kind="A", bias=True, norm=True, seed=0):
    """-> (Net, emb).  Probe A, narrow weights, exact in all three precisions: W1 integers in [-3, 3], b1 = k + 1/8; W2..W4 sparse, 4-8
    non-zeros per row from {+-1, +-2}; b2, b3, b4 = k + 2^-4, 2^-5, 2^-6; the embedding and W5 small integers, b5 half-integers;
    offset / scale absent or (integers, powers of two).

    Probe B, wide weights, exact on the f32-input matrix core only: probe A with the entries of ONE of W2..W4 (B2, B3, B4) of the form
    k / 16, |k| < 2^11 -- up to eleven significant bits, so their low bf16 half is not zero and a product needs the float32 multiplier.
    Wide weights in all three layers at once cannot be exact: each wide layer adds eleven bits to an activation and float32 holds 24,
    so the density is shrunk: one wide layer per probe with two non-zeros per row, two or three of +-1 per row in the other two, six
    per row in W5."""
    gen = torch.Generator().manual_seed(1000 + seed + 17 * PROBE_KINDS.index(kind))
    narrow = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)
    W = [_ints(gen, -3, 3, HIDDEN, 3)]
    for layer in (2, 3, 4):
        if kind == "A":
            W.append(_sparse(gen, narrow, 4, 8))
        elif kind == f"B{layer}":
            k = torch.arange(-(2 ** 11) + 1, 2 ** 11, dtype=torch.float64)
            W.append(_sparse(gen, k[k != 0] / 16.0, 2, 2))
        else:
            W.append(_sparse(gen, narrow[1:3], 2, 3))
    W.append(_ints(gen, -3, 3, 3, HIDDEN) if kind == "A" else _sparse(gen, narrow[1:3], 6, 6)[:3].contiguous())
    frac = (2.0 ** -3, 2.0 ** -4, 2.0 ** -5, 2.0 ** -6)
    b = [_ints(gen, -2, 2, HIDDEN) + f for f in frac] + [_ints(gen, -2, 2, 3) + 0.5]
    emb = _ints(gen, -2, 2, HIDDEN)
    net = Net(W, b if bias else [None] * 5, PROBE_OFFSET if norm else None, PROBE_SCALE if norm else None)
    return net, emb


PROBE_B_MARGIN = 1e-3
PROBE_POOL = 2048


def probe_points(kind, bias, norm, n, seed=0):
    """n inputs of probe(kind, bias, norm) whose normalised form is a multiple of 1/4 in [-2, 2] (xyz = xn * scale + offset, exact).
    Probe A takes the first n drawn.  Probe B also runs on the split planes, which are not exact on it: its inputs are the first n of
    a pool of 2048 at which every pre-activation is farther from zero than 1e-3 x its own mass (the sum of |w| |x| of its row plus
    |bias| and |embedding|: a split product errs by ~2^-16 of that; a row whose mass is zero is exactly zero in every arithmetic),
    and at which |o| >= 1 -- a choice of inputs, as in safe_points."""
    gen = torch.Generator().manual_seed(2000 + seed)
    m = max(n, PROBE_POOL)                # (a fixed pool: the inputs of a smaller n are a prefix of a larger n's)
    xyz = torch.randint(-8, 9, (m, 3), generator=gen).double() / 4.0
    if norm:
        xyz = xyz * torch.tensor(PROBE_SCALE, dtype=torch.float64) + torch.tensor(PROBE_OFFSET, dtype=torch.float64)
    if kind == "A":
        return xyz[:n].contiguous()
    net, emb = probe(kind, bias, norm)
    o, _, pres = sums(net, emb, xyz, torch.float64)
    ok = o.norm(dim=1) >= 1.0
    h = _norm_in(net, xyz, torch.float64)[0]
    for k, z in enumerate(pres):
        s = h.abs() @ net.W[k].abs().t() + (0.0 if net.b[k] is None else net.b[k].abs()) + (emb.abs() if k == 1 else 0.0)
        if k > 0:                       # (layer 1 is the same exact float32 sum in every precision)
            ok &= ((z.abs() > PROBE_B_MARGIN * s) | (s == 0)).all(dim=1)
        h = z.clamp_min(0)
    ok = torch.nonzero(ok)[:, 0]
    assert ok.numel() >= n, (kind, bias, norm, n, ok.numel())
    return xyz[ok[:n]].contiguous()


def significant_bits(x):
    """Largest count of significant bits (leading one to trailing one) over the entries of x (float64 holding float32 values)."""
    m, _ = np.frexp(np.abs(np.asarray(x, dtype=np.float64)).reshape(-1))
    m = m[m > 0]
    bits = np.zeros(m.shape, dtype=np.int64)
    left = np.ones(m.shape, dtype=bool)
    for k in range(1, 54):
        v = m * 2.0 ** k
        done = left & (v == np.floor(v))
        bits[done] = k
        left &= ~done
    assert not left.any()
    return int(bits.max()) if bits.size else 0


def fraction_bits(x):
    """Smallest f with x * 2^f integral everywhere."""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    for f in range(0, 60):
        if np.all(v * 2.0 ** f == np.floor(v * 2.0 ** f)):
            return f
    raise AssertionError("not dyadic")


def probe_conditions(net, emb, xyz, split_planes):
    """What makes the kernels' matrix products exact on this probe and these inputs -> a dict of the measured figures.
    operand_bits: significant bits of every matrix-core operand of the three 128 x 128 layers and of the output layer's activations, per
    plane kind; weight_bits: of W2..W4; sum_bits: log2 of the largest sum of |w| |x| of a row in units of the products' last place
    (every partial sum in any order is below it); near_zero: the smallest |pre-activation|; min_norm: the smallest |o|."""
    xn, inv = _norm_in(net, xyz, torch.float64)
    z = _layer1(net, xn, torch.float64)
    pres = [z]
    live = z > 0
    planes = [z * live] + [(net.W[0][:, j] * inv[j])[None, :] * live for j in range(3)]
    op_bits, sum_bits, split_ok = 0, 0.0, True
    for k in (1, 2, 3, 4):
        W = net.W[k]
        fw = fraction_bits(W)
        for t in range(4):
            X = planes[t]
            op_bits = max(op_bits, significant_bits(X))
            fx = fraction_bits(X)
            top = float((X.abs() @ W.abs().t()).max()) + (float(net.b[k].abs().max()) if net.b[k] is not None and t == 0 else 0.0) \
                + (float(emb.abs().max()) if k == 1 and t == 0 else 0.0)
            fsum = max(fw + fx, fraction_bits(net.b[k]) if net.b[k] is not None and t == 0 else 0)
            sum_bits = max(sum_bits, float(np.log2(max(top, 1e-300))) + fsum)
            if t in split_planes:            # (k = 4: the output layer reads the re-joined halves)
                split_ok &= bool(torch.equal(rejoin(X), X))
        if k == 4:
            break
        ys = [planes[t] @ W.t() for t in range(4)]
        z = _pre(ys[0], net.b[k], emb if k == 1 else None, torch.float64)
        pres.append(z)
        live = z > 0
        planes = [z * live] + [ys[t] * live for t in (1, 2, 3)]
    o = _pre(planes[0] @ net.W[4].t(), net.b[4], None, torch.float64)
    return {"operand_bits": op_bits, "weight_bits": max(significant_bits(net.W[k]) for k in (1, 2, 3)), "sum_bits": sum_bits,
            "split_is_exact": split_ok, "near_zero": min(float(p.abs().min()) for p in pres),
            "exact_zero_preactivations": int(sum(int((p == 0).sum()) for p in pres)), "min_norm": float(o.norm(dim=1).min())}


# ------------------------------------------------------------------------------------------------------------------ random nets
def fresh_net(seed=11, norm=True):
    """(Net, emb) of a fresh texgs.uvnet.UVNet initialisation."""
    from texgs.uvnet import UVNet
    torch.manual_seed(seed)
    kw = dict(xyz_offset=[0.1, -0.2, 0.05], xyz_scale=[1.5, 0.8, 1.2]) if norm else {}
    m = UVNet(precision="fp32", **kw)
    emb = (torch.randn(HIDDEN) * 0.2).double()
    return from_module(m), emb


def golden_net():
    """(Net, emb, xyz) of tests/golden/uvnet.npz: the reference's own UVNet."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvnet.npz"))
    W = [torch.tensor(G[f"{m}__{i}__weight"]) for m, i in (("pre_mlp", 0), ("pre_mlp", 2), ("mlp", 0), ("mlp", 2), ("mlp", 4))]
    b = [torch.tensor(G[f"{m}__{i}__bias"]) for m, i in (("pre_mlp", 0), ("pre_mlp", 2), ("mlp", 0), ("mlp", 2), ("mlp", 4))]
    return Net(W, b), torch.tensor(G["emb"]).double().reshape(-1), torch.tensor(G["xyz"]).double()


def rescaled(net, emb, seed=5):
    """The same function with ill-scaled rows, as a trained net has: row i of W2..W4 (with its bias, and the embedding on layer 2) times
    2^k, k uniform in [-6, 6], and column i of the next layer times 2^-k -- exact in binary, ReLU commutes with a positive factor."""
    gen = torch.Generator().manual_seed(seed)
    W, b, emb = [w.clone() for w in net.W], [None if x is None else x.clone() for x in net.b], emb.clone()
    for k in (1, 2, 3):
        s = 2.0 ** torch.randint(-6, 7, (HIDDEN,), generator=gen).double()
        W[k] = W[k] * s[:, None]
        if b[k] is not None:
            b[k] = b[k] * s
        if k == 1:
            emb = emb * s
        W[k + 1] = W[k + 1] / s[None, :]
    return Net(W, b, net.off, net.scale), emb


def candidates(n, seed):
    """The candidate inputs of safe_points: 4 n + 64 points near the unit sphere (radius 1 +- 2 %)."""
    gen = torch.Generator().manual_seed(seed)
    m = 4 * n + 64
    x = torch.randn(m, 3, generator=gen, dtype=torch.float64)
    x = x / x.norm(dim=1, keepdim=True) * (1 + 0.02 * torch.randn(m, 1, generator=gen, dtype=torch.float64))
    return x.float().double()


def safe_points(net, emb, n, rel_margin, seed=1):
    """The first n of 4 n + 64 candidates whose float64 pre-activations all lie farther than rel_margin x (the largest |pre-activation|
    of that layer and point) from zero; at least a quarter of the candidates must qualify, so the caller always gets n rows."""
    cand = candidates(n, seed)
    _, _, pres = sums(net, emb, cand, torch.float64)
    near = torch.stack([(z.abs() / z.abs().amax(dim=1, keepdim=True)).amin(dim=1) for z in pres], 0).amin(0)
    ok = torch.nonzero(near > rel_margin)[:, 0]
    assert 4 * ok.numel() >= cand.shape[0], (ok.numel(), cand.shape[0], rel_margin)
    return cand[ok[:n]].contiguous()
