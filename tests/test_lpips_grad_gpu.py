"""-m gpu: the backward of LPIPS-VGG on the device (csrc/lpips_grad.hip, texgs/lpips_grad.py, the chain of texgs/lpips.py) against the
float64 statement of tests/lpips_grad_ref.py.  The cases, their shared CPU evaluations and the NaN-guarded buffers are stated in
tests/lpips_grad_cases.py.

Yardstick, for every compared map: max |hip - f64| <= 4 max(max |f32 - f64|, 2^-23 max |f64|), the project's bound for this stage
(lpips_ref.tolerance), where f32 is the statement's own loops in float32.  All three evaluations take the activations read back from
the GPU forward, so no ReLU mask and no pool arg-max is left to disagree on and no element is excluded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as C  # noqa: E402
import lpips_grad_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu


def _within(name, e, y):
    print(f"{name}: max|hip - f64| = {e:.3e}, yardstick {y:.3e}, ratio {e / y if y else 0.0:.3f} (bound {GC.BOUND})")
    assert e <= GC.BOUND * y, name


# ---- the head's backward alone ----
@pytest.mark.parametrize("i", range(len(GC.HEAD_BWD_CASES)), ids=[GC.head_id(c) for c in GC.HEAD_BWD_CASES])
def test_head_backward_against_the_statement(lib_built, i):
    for wrt in (1, 2, 3):
        e, y = GC.measure_head_backward(i, wrt)
        _within(f"head backward {GC.head_id(GC.HEAD_BWD_CASES[i])} wrt={wrt}", e, y)


def test_head_backward_rules_on_planted_maps(lib_built):
    """Equal maxima: the first in row-major order takes the gradient; an all-zero window and a zero pixel take nothing; the odd last
    row and column get the head term only"""
    i = len(GC.HEAD_BWD_CASES) - 1
    d = GC.head_bwd_case(i)
    got, _ = GC.run_head_backward(d, 3)
    got = got.cpu().numpy()
    zero_next = dict(d, g_next=np.zeros_like(d["g_next"]))
    head_only, _ = GC.run_head_backward(zero_next, 3)
    routed = got - head_only.cpu().numpy()                               # what the unpool added, where the gate is open
    gn = d["g_next"]
    assert np.array_equal(got[:, :, 36, :], head_only.cpu().numpy()[:, :, 36, :]) and np.array_equal(got[:, :, :, 40], head_only.cpu().numpy()[:, :, :, 40])
    assert np.abs(routed[:, :, 4, 6] - gn[:, :, 2, 3]).max() < 1e-5 and not routed[:, :, 4:6, 7].any() and not routed[:, :, 5, 6].any()
    assert np.abs(routed[:, :, 10, 13] - gn[:, :, 5, 6]).max() < 1e-5 and not routed[:, :, 11, 12].any()
    assert np.abs(routed[:, :, 11, 14] - gn[:, :, 5, 7]).max() < 1e-5 and not routed[:, :, 11, 15].any()
    assert not got[:, :, 20:24, 20:26].any()
    zp = GC.head_bwd_case([k for k, c in enumerate(GC.HEAD_BWD_CASES) if c == (6, True, False)][0])       # the zero-pixel case
    g, _ = GC.run_head_backward(zp, 3)
    assert not bool(g[:, :, 1, 2].any()) and bool(torch.isfinite(g).all())


def test_head_backward_swapped_pair_and_repeat_are_bit_identical(lib_built):
    from texgs import lpips_grad as G
    d = GC.head_bwd_case(len(GC.HEAD_BWD_CASES) - 1)
    P = d["f"].shape[0] // 2
    f, lin, gbar, gn = C.cuda(d["f"]), C.cuda(d["lin"]), C.cuda(d["gbar"]), C.cuda(d["g_next"])
    a = G.head_backward(f, lin, gbar, 3, g_next=gn)
    b = G.head_backward(f, lin, gbar, 3, g_next=gn)
    swapped = G.head_backward(torch.cat([f[P:], f[:P]]), lin, gbar, 3, g_next=torch.cat([gn[P:], gn[:P]]))
    only1 = G.head_backward(f, lin, gbar, 1, g_next=gn[:P].contiguous())
    only2 = G.head_backward(f, lin, gbar, 2, g_next=gn[P:].contiguous())
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(swapped[:P]), bits(a[P:])) and torch.equal(bits(swapped[P:]), bits(a[:P]))
    assert torch.equal(bits(only1), bits(a[:P])) and torch.equal(bits(only2), bits(a[P:]))


# ---- the gate ----
@pytest.mark.parametrize("n", GC.GATE_COUNTS)
def test_gate_is_exact_at_any_count(lib_built, n):
    g, y, want = GC.gate_case(n)
    got = GC.run_gate(g, y).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))       # +0 where the gate is closed, G's bits where it is open
    assert (np.signbit(y) & (y == 0)).any() or n == 3


# ---- the transposed weights through the forward's convolution ----
@pytest.mark.parametrize("i", range(len(GC.CONVT_CASES)), ids=["%d-%dx%dx%dx%d" % c for c in GC.CONVT_CASES])
def test_transposed_weights_give_the_data_gradient(lib_built, i):
    e, y = GC.measure_convt(i)
    _within(f"transposed convolution {GC.CONVT_CASES[i]}", e, y)


# ---- the whole chain ----
@pytest.mark.parametrize("size", GC.CHAIN_SIZES, ids=["%dx%d" % s for s in GC.CHAIN_SIZES])
def test_chain_against_the_statement_on_the_gpus_own_activations(lib_built, size):
    d = GC.chain_case(size)
    assert len(d["maps"]) == 13 and d["maps"][0].shape == (4, 64) + size
    for wrt in (1, 2, 3):
        for which, e, y in GC.measure_chain(size, wrt):
            _within(f"chain {size} wrt={wrt} d {which}", e, y)


# ---- through the public surface ----
def test_backward_fills_the_grad_and_the_value_is_the_no_grad_value(lib_built):
    net, _, _ = C.net()
    img0_np, img1_np, _ = GC.chain_inputs((17, 31))
    img0, img1 = C.cuda(img0_np), C.cuda(img1_np)
    plain = net(img0, img1, normalize=True)
    assert not plain.requires_grad
    img0.requires_grad_()
    v = net(img0, img1, normalize=True)
    assert v.requires_grad and tuple(v.shape) == (2, 1, 1, 1) and torch.equal(v.detach().view(torch.int32), plain.view(torch.int32))
    v.sum().backward()
    assert img0.grad is not None and img0.grad.shape == img0.shape and img0.grad.dtype == torch.float32 and img1.grad is None
    assert bool(torch.isfinite(img0.grad).all()) and float(img0.grad.abs().max()) > 0
    # sum(): gbar = 1 for both pairs -- the chain's own result
    state = net._forward_grad(img0.detach(), img1, True)[1]
    d0, d1 = net._backward_grad(state, torch.ones(2, device="cuda"), 1)
    assert d1 is None and torch.equal(d0.view(torch.int32), img0.grad.view(torch.int32))
    # the no-grad surfaces still run, and do not keep a graph
    with torch.no_grad():
        assert torch.equal(net(img0, img1, normalize=True), plain)
    assert not net.table(img0, img1, normalize=True).requires_grad
    # a descent step along the gradient lowers the value
    with torch.no_grad():
        stepped = net((img0 - 0.01 * img0.grad / img0.grad.abs().max()).clamp(0, 1), img1, normalize=True)
    assert float(stepped.sum()) < float(plain.sum())
    # both inputs, unbatched, a weighted sum
    a, b = C.cuda(img0_np[0]).requires_grad_(), C.cuda(img1_np[0]).requires_grad_()
    (net(a, b, normalize=True) * 1.5).sum().backward()
    assert a.grad.shape == a.shape and b.grad.shape == b.shape and float(b.grad.abs().max()) > 0
    v = net(a, b, normalize=True).sum()
    v.backward()
    with pytest.raises(RuntimeError, match="second time"):
        v.backward()
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(net(a, b).sum(), a, create_graph=True)


def test_dropin_is_differentiable_with_weights_from_files(lib_built, tmp_path):
    from texgs import lpips as L
    import lpips
    net, _, _ = C.net()
    torch.save({f"features.{i}.{leaf}": t for i, (w, b) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", b))},
               tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}, tmp_path / "lin.pth")
    with pytest.warns(RuntimeWarning, match="UNPINNED"):
        m = lpips.LPIPS(net="vgg", model_path=str(tmp_path / "lin.pth"), vgg_path=str(tmp_path / "vgg16.pth"), verbose=False).to("cuda")
    img0_np, img1_np, _ = GC.chain_inputs((16, 16))
    render, gt = C.cuda(img0_np).requires_grad_(), C.cuda(img1_np)
    m(render, gt, normalize=True).sum().backward()
    ours = C.cuda(img0_np).requires_grad_()
    net(ours, gt, normalize=True).sum().backward()
    assert render.grad is not None and torch.equal(render.grad.view(torch.int32), ours.grad.view(torch.int32)) and float(ours.grad.abs().max()) > 0


# ---- bit-level properties of the chain ----
def test_chain_bits_repeat_slot_and_swap(lib_built):
    net, _, _ = C.net()
    img0_np, img1_np, gbar_np = GC.chain_inputs((17, 31))
    a, b, gbar = C.cuda(img0_np), C.cuda(img1_np), C.cuda(gbar_np)
    bits = lambda t: t.contiguous().view(torch.int32)

    def grads(x0, x1, g, wrt=3):
        return net._backward_grad(net._forward_grad(x0, x1, True)[1], g, wrt)
    d0, d1 = grads(a, b, gbar)
    e0, e1 = grads(a, b, gbar)
    assert torch.equal(bits(d0), bits(e0)) and torch.equal(bits(d1), bits(e1))                   # two backwards, equal bits
    s0, s1 = grads(b, a, gbar)                                                                     # d img1 of (a, b) = d img0 of (b, a)
    assert torch.equal(bits(s0), bits(d1)) and torch.equal(bits(s1), bits(d0))
    o0, none = grads(a, b, gbar, 1)                                                                # one side alone: the same bits
    assert none is None and torch.equal(bits(o0), bits(d0))
    none, o1 = grads(a, b, gbar, 2)
    assert none is None and torch.equal(bits(o1), bits(d1))
    # a pair's gradient is the same in any batch slot: pair 1 alone, and as slot 0 and slot 2 of three pairs
    p0, p1 = grads(a[1:], b[1:], gbar[1:])
    assert torch.equal(bits(p0), bits(d0[1:])) and torch.equal(bits(p1), bits(d1[1:]))
    three = lambda t: torch.cat([t[1:], t[:1], t[1:]])
    t0, t1 = grads(three(a), three(b), three(gbar))
    for k in (0, 2):
        assert torch.equal(bits(t0[k]), bits(d0[1])) and torch.equal(bits(t1[k]), bits(d1[1]))
    assert torch.equal(bits(t0[1]), bits(d0[0]))
