"""tests/uvnet_ref.py checked on the host: the statement the row-by-row GPU tests of the UV-net kernels (tests/test_uvnet_rows_gpu.py)
compare against is the network of texgs.uvnet, its scales are the sums they say they are, the probe networks are exact where the
GPU tests assume exactness, and the input selections always fill their quota."""
import os

import numpy as np
import pytest
import torch

from texgs.uvnet import UVNet, jacobian_by_autograd, uvnet_backward
import uvnet_ref as R


def _module(net):
    kw = {} if net.off is None else dict(xyz_offset=net.off.tolist(), xyz_scale=net.scale.tolist())
    m = UVNet(precision="fp32", **kw).double()
    with torch.no_grad():
        for lin, w, b in zip(m._linears(), net.W, net.b):
            lin.weight.copy_(w)
            lin.bias.zero_() if b is None else lin.bias.copy_(b)
    return m


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _cases():
    net, emb = R.fresh_net(11, True)
    yield "fresh", net, emb, R.candidates(10, 3)[:50]
    net, emb = R.fresh_net(12, False)
    yield "fresh_plain", net.without_bias(), emb, R.candidates(10, 4)[:50]
    net, emb = R.rescaled(*R.fresh_net(11, True))
    yield "rescaled", net, emb, R.candidates(10, 3)[:50]
    net, emb, xyz = R.golden_net()
    yield "golden", net, emb, xyz[:50]


@pytest.mark.parametrize("name", ["fresh", "fresh_plain", "rescaled", "golden"])
def test_statement_is_the_module_in_float64(name):
    """forward = UVNet.forward and jacobian_by_autograd, backward = uvnet_backward (itself checked against autograd in test_uvnet.py),
    to 1e-10 relative -- a NULL bias is a zero bias; on the golden file also the reference's own uvs and Jacobian."""
    net, emb, xyz = next(c[1:] for c in _cases() if c[0] == name)
    m = _module(net)
    uvs, J = R.forward(net, emb, xyz, torch.float64)
    with torch.no_grad():
        want_uv = m(xyz, emb)
    assert _rel(uvs, want_uv) < 1e-10
    assert _rel(J, jacobian_by_autograd(m, xyz, emb)) < 1e-10
    if name == "golden":
        G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvnet.npz"))
        assert float((uvs - torch.tensor(G["uvs"])[:50]).abs().max()) < 5e-7            # (the reference casts to float32 on its way)
        assert _rel(J, torch.tensor(G["J"])[:50]) < 1e-5
    g = torch.randn(xyz.shape[0], 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = R.backward(net, emb, xyz, g, torch.float64)
    lins = m._linears()
    with torch.no_grad():
        _, demb, dW, db = uvnet_backward(m._norm_in(xyz), emb, [l.weight for l in lins], [l.bias for l in lins], g)
    for k in range(5):
        assert _rel(got[f"W{k + 1}"], dW[k]) < 1e-10 and _rel(got[f"b{k + 1}"], db[k]) < 1e-10, k
    assert _rel(got["b2"], demb) < 1e-10


def test_rescaled_net_is_the_same_function_bit_for_bit():
    net, emb = R.fresh_net(11, True)
    net2, emb2 = R.rescaled(net, emb)
    xyz = R.candidates(10, 3)
    a, b = R.forward(net, emb, xyz, torch.float64), R.forward(net2, emb2, xyz, torch.float64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ratio = net2.W[2].abs().amax(dim=1) / net.W[2].abs().amax(dim=1)
    assert float(ratio.max() / ratio.min()) >= 1024.0                         # rows three orders of magnitude apart


def test_scales_are_brute_force_sums_per_point():
    """N = 8: every S entry is the sum over the points of (addends of d, in absolute value) x (addends of h, in absolute value), and the
    plain scale the sum of |d h|; each is at least the |gradient| it measures, and zero only where the gradient is exactly zero."""
    net, emb = R.fresh_net(11, True)
    xyz = R.candidates(8, 5)[:8]
    g = torch.randn(8, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out, S, Sp = R.backward(net, emb, xyz, g, torch.float64, scales=True)
    acc = {k: torch.zeros_like(v) for k, v in S.items()}
    accp = {k: torch.zeros_like(v) for k, v in S.items()}
    total = {k: torch.zeros_like(v) for k, v in S.items()}
    for p in range(8):
        o1, S1, Sp1 = R.backward(net, emb, xyz[p:p + 1], g[p:p + 1], torch.float64, scales=True)
        for k in S:
            acc[k] += S1[k]
            accp[k] += o1[k].abs()                    # one point: an entry IS its one term
            total[k] += o1[k]
            assert torch.allclose(Sp1[k], o1[k].abs(), rtol=1e-12, atol=0)
    for k in S:
        assert torch.allclose(S[k], acc[k], rtol=1e-12, atol=0), k
        assert torch.allclose(Sp[k], accp[k], rtol=1e-12, atol=0), k
        assert torch.allclose(out[k], total[k], rtol=1e-9, atol=1e-300), k
        assert bool((S[k] >= Sp[k] * (1 - 1e-12)).all()) and bool((Sp[k] >= out[k].abs() * (1 - 1e-12)).all()), k
        assert bool(((S[k] == 0) == (Sp[k] == 0)).all()), k


def test_scales_against_a_loop_over_the_addends():
    """The scale S the GPU tests divide by, re-derived without uvnet_ref's formulas: numpy, one point at a time, every sum as a loop over
    its addends j -- own(i) += |addend j|, carried(i) += (scale of j)^2 w_ji^2, scale = sqrt(own^2 + carried) under the unit's mask --
    down the chain for d and up the chain for h, then S = sum over points of scale_d x scale_h.  Every entry of all ten, N = 5, with
    offset / scale and biases; a wrong mask, weight or factor in uvnet_ref.backward's m_k / a_k shows here."""
    net, emb = R.fresh_net(11, True)
    n = 5
    xyz = R.candidates(8, 5)[:n]
    g = torch.randn(n, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    _, S, _ = R.backward(net, emb, xyz, g, torch.float64, scales=True)
    W = [w.numpy() for w in net.W]
    b = [x.numpy() for x in net.b]
    want = {k: np.zeros(R.SHAPES[k]) for k in R.NAMES}

    def carry(addends, scales, w_rows, extra, live):           # w_rows[j] = the weights unit j contributes through, one per output unit
        own, up = np.array(extra, dtype=np.float64), np.zeros_like(extra)
        for j in range(len(addends)):
            own = own + abs(addends[j]) * np.abs(w_rows[j])
            up = up + scales[j] ** 2 * w_rows[j] ** 2
        return np.sqrt(own ** 2 + up) * live

    for p in range(n):
        x = (xyz[p].numpy() - net.off.numpy()) / net.scale.numpy()
        h, z, a = [x], [], [(np.abs(xyz[p].numpy()) + np.abs(net.off.numpy())) / np.abs(net.scale.numpy())]
        for k in range(5):
            zk = W[k] @ h[k] + b[k] + (emb.numpy() if k == 1 else 0.0)
            live = (zk > 0) if k < 4 else np.ones(3)
            extra = np.abs(b[k]) + (np.abs(emb.numpy()) if k == 1 else 0.0)
            a.append(carry(h[k], a[k] if k > 0 else np.zeros(3), W[k].T, extra, live) if k > 0
                     else (np.abs(W[0]) @ a[0] + extra) * live)
            z.append(zk)
            h.append(np.maximum(zk, 0.0) if k < 4 else zk)
        o = h[5]
        nrm = np.sqrt((o ** 2).sum())
        u = o / nrm
        gp = g[p].numpy()
        d = {5: (gp - u * (u * gp).sum()) / nrm}
        m = {5: max(a[5].sum() / nrm, 1.0) * (np.abs(gp) + np.abs(u) * (np.abs(u) * np.abs(gp)).sum()) / nrm}
        for k in (4, 3, 2, 1):                                   # d_k = (W_{k+1}^T d_{k+1}) . [z_k > 0]
            live = z[k - 1] > 0
            d[k] = (W[k].T @ d[k + 1]) * live
            m[k] = carry(d[k + 1], m[k + 1], W[k], np.zeros(W[k].shape[1]), live)
        for k in (1, 2, 3, 4, 5):
            want[f"W{k}"] += np.outer(m[k], a[k - 1])
            want[f"b{k}"] += m[k]
    for k in R.NAMES:
        assert np.allclose(S[k].numpy(), want[k], rtol=1e-12, atol=0), k


def test_kernel_order_normalise_is_the_same_mathematics():
    """finish_kernel_order (float32, uv_finish's operation order) against the float64 normalise step: a few roundings per row, and
    not torch's float32 bits -- which is why the GPU test compares the kernel's bits with IT and holds torch's to the bar."""
    net, emb = R.probe("A", True, True)
    o, dO, _ = R.sums(net, emb, R.probe_points("A", True, True, 129), torch.float64)
    uv64, J64 = R.finish(o, dO, torch.float64)
    uk, Jk = R.finish_kernel_order(o, dO)
    ut, Jt = R.finish(o, dO, torch.float32)
    assert uk.dtype == torch.float32 and float(R.row_error(uk, uv64).max()) < 4 * R.FLOOR
    assert float(R.row_error(Jk, J64).max()) <= 4 * max(float(R.row_error(Jt, J64).max()), R.FLOOR)
    assert not R.same_bits(uk, ut)


def test_plain_scale_is_no_yardstick_where_a_factor_cancels():
    """Why the scale carries the addends of d and h and not |d| |h|: two float32 evaluations of the SAME chain that differ only in the
    order of the hidden neurons (so in summation order) are, in units of |d|^T |h|, thousands of roundings from float64 at their worst
    entry -- an entry whose h or d is the small remainder of a cancelling sum -- while in units of the addends both are a few 2^-24."""
    net, emb = R.fresh_net(11, True)
    xyz = R.safe_points(net, emb, 200, 1e-5, seed=1)
    g = torch.randn(200, 3, generator=torch.Generator().manual_seed(0)).double()
    ref, S, Sp = R.backward(net, emb, xyz, g, torch.float64, scales=True)
    st = R.backward(net, emb, xyz, g, torch.float32)
    plain = max(R.entry_error(st[k], ref[k], Sp[k]) for k in R.NAMES)
    mass = max(R.entry_error(st[k], ref[k], S[k]) for k in R.NAMES)
    assert plain > 1000 * R.FLOOR and mass < 32 * R.FLOOR, (plain, mass)


def test_no_split_planes_is_the_float32_path_bit_for_bit():
    net, emb = R.fresh_net(11, True)
    xyz = R.candidates(10, 3)
    f32 = torch.float32
    xn = (xyz.to(f32) - net.off.to(f32)) * (1.0 / net.scale.to(f32))
    W, b = [w.to(f32) for w in net.W], [x.to(f32) for x in net.b]
    z = ((b[0] + xn[:, 0:1] * W[0][:, 0]) + xn[:, 1:2] * W[0][:, 1]) + xn[:, 2:3] * W[0][:, 2]
    h = z.clamp_min(0)
    h = ((h @ W[1].t() + b[1]) + emb.to(f32)).clamp_min(0)
    h = (h @ W[2].t() + b[2]).clamp_min(0)
    h = (h @ W[3].t() + b[3]).clamp_min(0)
    o = h @ W[4].t() + b[4]
    u = o / o.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    got, _ = R.forward(net, emb, xyz, f32, ())
    assert got.dtype == f32 and R.same_bits(got, u)
    # and a split plane is another arithmetic: ~2^-17, not float32's 2^-24
    _, J0 = R.forward(net, emb, xyz, f32, ())
    uv1, J1 = R.forward(net, emb, xyz, f32, (1, 2, 3))
    assert R.same_bits(uv1, got) and not R.same_bits(J1, J0)
    assert 1e-7 < float(R.row_error(J1, J0).max()) < 1e-3
    hi, lo = R.split_bf16(torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -20]))
    assert float(hi) == 1.0 and float(lo) == 2.0 ** -9


@pytest.mark.parametrize("kind", R.PROBE_KINDS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("norm", [True, False])
def test_probe_conditions(kind, bias, norm):
    """What the GPU tests take for granted on the shipped probes and their 129 inputs: matrix-core operands of at most 16 significant
    bits with x == bf16(x) + bf16(x - bf16(x)) and weights of at most 8 on probe A (no lo.lo term exists), wider weights on probe B;
    every partial sum of every row below 2^24 units of its last place; with biases no pre-activation within 2^-7 of zero (without
    them a pre-activation may BE zero: it is then an exact zero in every arithmetic, dead in the kernels and in the statement
    alike); |o| >= 1; and, the consequence, o and dO of the float32 statement -- split planes included on probe A -- equal to float64."""
    net, emb = R.probe(kind, bias, norm)
    xyz = R.probe_points(kind, bias, norm, 129)
    assert xyz.shape == (129, 3) and torch.equal(xyz[:33], R.probe_points(kind, bias, norm, 33))
    xn = R._norm_in(net, xyz, torch.float64)[0]
    assert float(xn.abs().max()) <= 2.0 and torch.equal(xn * 4, (xn * 4).round())
    c = R.probe_conditions(net, emb, xyz, (0, 1, 2, 3) if kind == "A" else ())
    assert c["sum_bits"] < 24.0, c
    assert c["min_norm"] >= 1.0, c
    if bias:
        assert c["near_zero"] >= 2.0 ** -7 and c["exact_zero_preactivations"] == 0, c
    if kind == "A":
        assert c["operand_bits"] <= 16 and c["weight_bits"] <= 8 and c["split_is_exact"], c
        if bias:
            assert c["min_norm"] > 500.0, c
    else:
        assert 8 < c["weight_bits"] <= 12, c
    o64, d64, _ = R.sums(net, emb, xyz, torch.float64)
    for planes in ((), (1, 2, 3), (0, 1, 2, 3)) if kind == "A" else ((),):
        o32, d32, _ = R.sums(net, emb, xyz, torch.float32, planes)
        assert torch.equal(o32.double(), o64) and torch.equal(d32.double(), d64), planes
    if kind != "A":                                   # the value column of "mixed" is the float32 one
        o32, d32, _ = R.sums(net, emb, xyz, torch.float32, (1, 2, 3))
        assert torch.equal(o32.double(), o64)
        # (whether a split plane is exact on a probe B -- its activations may or may not have a low half for the wide weights' low half
        #  to meet -- is read off the statement case by case in the GPU tests, never assumed)


def test_probe_a_stays_exact_at_the_backward_sizes():
    net, emb = R.probe("A", True, True)
    xyz = R.probe_points("A", True, True, 16_450)
    c = R.probe_conditions(net, emb, xyz, ())
    assert c["sum_bits"] < 24.0 and c["near_zero"] >= 2.0 ** -7 and c["min_norm"] > 100.0, c


@pytest.mark.parametrize("which", ["fresh", "golden"])
def test_safe_points_quotas(which):
    """At least a quarter of the 4 n + 64 candidates qualify at both margins (asserted inside), so n rows always come back, and they
    are what they claim: every float64 pre-activation beyond the margin.  (The rescaled net takes the fresh net's points: its
    pre-activations are the fresh net's times a power of two per row, so is every rounding error of a row, and a margin measured
    against the largest row of a layer would only measure the row scales.)"""
    if which == "golden":
        net, emb, _ = R.golden_net()
    else:
        net, emb = R.fresh_net(11, True)
        net2, emb2 = R.rescaled(net, emb)
        xyz = R.safe_points(net, emb, 33, 1e-5)
        for z, z2 in zip(R.sums(net, emb, xyz, torch.float64)[2][1:], R.sums(net2, emb2, xyz, torch.float64)[2][1:]):
            s = z2 / z
            assert bool((s == s[0:1]).all()) and torch.equal(torch.log2(s[0]), torch.log2(s[0]).round())
    for n, margin in ((33, 1e-5), (200, 1e-5), (33, 1e-3), (200, 1e-3), (97, 1e-3)):
        xyz = R.safe_points(net, emb, n, margin)
        assert xyz.shape == (n, 3) and torch.equal(xyz.float().double(), xyz)
        _, _, pres = R.sums(net, emb, xyz, torch.float64)
        for z in pres:
            assert bool((z.abs() > margin * z.abs().amax(dim=1, keepdim=True)).all())
