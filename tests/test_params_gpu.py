"""-m gpu: the parameter stage on the device (texgs/params.py, csrc/params.hip) against the numpy statements of tests/params_ref.py.

The float64 statement is the truth; the float32 statement, with the kernels' operation order, sets the bound: a field's error
(max |device - float64| / scale, no element excluded) may be at most PARITY_FACTOR x the float32 statement's own, floored at 2^-24.
`rotations` holds no transcendental and is compared with the float32 statement bit for bit; so are the special rows, by class and,
where finite, by bits."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import params_ref as R  # noqa: E402
from texgs import params as P  # noqa: E402

pytestmark = pytest.mark.gpu
RPW = P.ROWS_PER_WORKGROUP
SIZES = [1, 2, 63, 64, 65, RPW - 1, RPW, RPW + 1, 3 * RPW + 5]          # the reduce sees one, two and four partials
EPS = 1e-3
MOD = 0.37
DEV = "cuda:0"


def dev(x, grad=False):
    return torch.tensor(np.asarray(x, R.F), device=DEV).requires_grad_(grad)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(N, seed=11):
    """Inputs, upstream gradients and both statements of one size: computed once, shared, never modified"""
    a, q, x = R.random_rows(N, seed + N)
    g = R.random_grads(N, seed + N)
    return a, q, x, g, R.parity_fields(a, q, x, g, EPS, MOD)


def run_device(a, q, x, g, epsilon=EPS, modifier=MOD, want=(True, True, True), drop=()):
    """activate (+ reg) and covariance, forward and backward, with the weighted-sum losses whose upstream gradients are exactly g"""
    ta, tq, tx = dev(a, want[0]), dev(q, want[1]), dev(x, want[2])
    s, r, o, reg = P.activate(ta, tq, tx, opacity_reg=True, epsilon=epsilon)
    parts = {"g_scales": lambda: (s * dev(g["g_scales"])).sum(), "g_rotations": lambda: (r * dev(g["g_rotations"])).sum(),
             "g_opacities": lambda: (o * dev(g["g_opacities"])).sum(), "g_reg": lambda: reg * float(g["g_reg"])}
    loss = sum(f() for k, f in parts.items() if k not in drop)
    out = dict(scales=host(s), rotations=host(r), opacities=host(o), reg=host(reg).reshape(1))
    if any(want):
        loss.backward()
    out.update(d_scaling=host(ta.grad), d_rotation=host(tq.grad), d_opacity=host(tx.grad))
    ca, cq = dev(a, True), dev(q, True)
    cov = P.covariance(ca, cq, modifier)
    (cov * dev(g["g_cov"])).sum().backward()
    out.update(cov=host(cov), cov_d_scaling=host(ca.grad), cov_d_rotation=host(cq.grad))
    return out


@pytest.mark.parametrize("N", SIZES)
def test_parity_with_the_float64_statement_at_every_size(N):
    a, q, x, g, fields = case(N)
    got = run_device(a, q, x, g)
    ratios = {}
    for name, (truth, stated, scale) in fields.items():
        e_dev = R.max_error(got[name], truth, scale)
        e_ref = max(R.max_error(stated, truth, scale), R.PARITY_FLOOR)
        ratios[name] = e_dev / e_ref
        print(f"N={N} {name}: device {e_dev:.3e}, float32 statement {e_ref:.3e}, ratio {ratios[name]:.3f}, "
              f"bits equal: {R.same_class_and_bits(got[name], np.asarray(stated).reshape(np.asarray(got[name]).shape))}")
    print("PARITY", json.dumps({"N": N, "ratios": ratios}))
    for name, ratio in ratios.items():
        assert ratio <= R.PARITY_FACTOR, (name, ratio)
    assert np.array_equal(got["rotations"].view(np.uint32), fields["rotations"][1].view(np.uint32))        # no transcendental: bit for bit


def test_special_rows_have_the_class_and_bits_of_the_float32_statement():
    a, q, x = R.special_rows(EPS)
    N = a.shape[0]
    g = R.random_grads(N, seed=2)
    got = run_device(a, q, x, g)
    f = R.S32.activate(a, q, x, EPS)
    b = R.S32.activate_backward(q, f["scales"], f["opacities"], g["g_scales"], g["g_rotations"], g["g_opacities"], g["g_reg"], EPS)
    cb = R.S32.covariance_backward(a, q, MOD, g["g_cov"])
    want = dict(scales=f["scales"], rotations=f["rotations"], opacities=f["opacities"].reshape(-1, 1), d_scaling=b[0], d_rotation=b[1],
                d_opacity=b[2].reshape(-1, 1), cov=R.S32.covariance(a, q, MOD), cov_d_scaling=cb[0], cov_d_rotation=cb[1])
    for name, w in want.items():
        assert R.same_class_and_bits(got[name], w), (name, got[name], w)
    assert np.isinf(got["scales"]).any() and (got["scales"] == 0).any() and (got["opacities"] == 0).any() and (got["opacities"] == 1).any()
    assert (got["rotations"][2] == 0).all() and not np.isfinite(got["cov"][0]).any()
    # the clamp's inclusive edges, exactly: epsilon and 1 - epsilon and their neighbours as the saved opacities of the backward
    o = R.edge_opacities(EPS)
    go = np.linspace(-1, 1, o.size).astype(R.F)
    greg = R.F(1.5)
    d = P._activate_backward_raw(torch.device(DEV), o.size, None, None, dev(o), None, None, dev(go), dev(greg), EPS, (False, False, True))[2]
    w = R.S32.activate_backward(np.ones((o.size, 4)), np.ones((o.size, 3)), o, None, None, go, greg, EPS)[2]
    assert R.same_class_and_bits(host(d), w)
    only_reg = P._activate_backward_raw(torch.device(DEV), o.size, None, None, dev(o), None, None, None, dev(greg), EPS, (False, False, True))[2]
    assert np.array_equal(host(only_reg) != 0, [False, True, True, True, True, False])


@pytest.mark.parametrize("drop", ["g_scales", "g_rotations", "g_opacities", "g_reg"])
def test_an_absent_upstream_gradient_is_a_zero_gradient(drop):
    N = RPW + 1
    a, q, x, g, _ = case(N)
    got = run_device(a, q, x, g, drop=(drop,))
    f = R.S32.activate(a, q, x, EPS)
    kw = {k: (None if k == drop else g[k]) for k in ("g_scales", "g_rotations", "g_opacities", "g_reg")}
    want = R.S32.activate_backward(q, f["scales"], f["opacities"], epsilon=EPS, **kw)
    for name, w in zip(("d_scaling", "d_rotation", "d_opacity"), want):
        assert R.same_class_and_bits(got[name].reshape(w.shape), w), name
    zero = {"g_scales": "d_scaling", "g_rotations": "d_rotation"}.get(drop)
    if zero:
        assert not got[zero].any()


@pytest.mark.parametrize("unwanted", [0, 1, 2])
def test_an_input_that_does_not_require_grad_gets_none(unwanted):
    N = 65
    a, q, x, g, _ = case(N)
    want = tuple(i != unwanted for i in range(3))
    before = P.BACKWARD_CALLS["activate"]
    got = run_device(a, q, x, g, want=want)
    assert P.BACKWARD_CALLS["activate"] == before + 1
    full = run_device(a, q, x, g)
    for i, name in enumerate(("d_scaling", "d_rotation", "d_opacity")):
        if i == unwanted:
            assert got[name] is None
        else:
            assert np.array_equal(got[name].view(np.uint32), full[name].view(np.uint32)), name
    # the covariance likewise
    for wa, wq in ((True, False), (False, True)):
        ca, cq = dev(a, wa), dev(q, wq)
        (P.covariance(ca, cq, MOD) * dev(g["g_cov"])).sum().backward()
        assert (ca.grad is None) == (not wa) and (cq.grad is None) == (not wq)
        assert np.array_equal(host(ca.grad if wa else cq.grad), full["cov_d_scaling" if wa else "cov_d_rotation"])


def test_two_consumers_one_backward_launch():
    N = 3 * RPW + 5
    a, q, x, g, _ = case(N)
    g2 = R.random_grads(N, seed=77)
    ta, tq, tx = dev(a, True), dev(q, True), dev(x, True)
    s, r, o = P.activate(ta, tq, tx)
    loss = sum((t * dev(u[k])).sum() for u in (g, g2) for t, k in ((s, "g_scales"), (r, "g_rotations"), (o, "g_opacities")))
    before = P.BACKWARD_CALLS["activate"]
    loss.backward()
    assert P.BACKWARD_CALLS["activate"] == before + 1
    f = R.S32.activate(a, q, x)
    want = R.S32.activate_backward(q, f["scales"], f["opacities"], g["g_scales"] + g2["g_scales"], g["g_rotations"] + g2["g_rotations"],
                                   g["g_opacities"] + g2["g_opacities"], None)
    for t, w, name in zip((ta, tq, tx), want, ("d_scaling", "d_rotation", "d_opacity")):
        assert R.same_class_and_bits(host(t.grad).reshape(w.shape), w), name


def test_determinism_across_calls_and_positions():
    N = 1000
    a, q, x, g, _ = case(N)
    one, two = run_device(a, q, x, g), run_device(a, q, x, g)
    for k in one:
        assert np.array_equal(one[k].view(np.uint32), two[k].view(np.uint32)), k
    i = 300
    g1 = {k: (v if k == "g_reg" else v[i:i + 1]) for k, v in g.items()}
    # (the regulariser's gradient carries 1 / N, so it is left out of the position check; reg itself is a mean over other rows)
    big = run_device(a, q, x, g, drop=("g_reg",))
    row = run_device(a[i:i + 1], q[i:i + 1], x[i:i + 1], g1, drop=("g_reg",))
    for k in row:
        if k != "reg":
            assert np.array_equal(row[k][0].view(np.uint32), big[k][i].view(np.uint32)), k


@pytest.mark.parametrize("N", [1, RPW + 1, 3 * RPW + 5, 70001])
def test_regulariser_against_float64_and_on_its_own(N):
    a, q, x, g, fields = case(N) if N <= 3 * RPW + 5 else (*R.random_rows(N, 5), None, None)
    tx = dev(x, True)
    reg4 = P.activate(dev(a), dev(q), tx, opacity_reg=True, epsilon=EPS)[3]
    t64, t32 = R.S64.activate(a, q, x, EPS), R.S32.activate(a, q, x, EPS)
    truth = float(t64["reg"])
    e_dev = abs(float(reg4) - truth) / abs(truth)
    e_ref = max(abs(float(t32["reg"]) - truth) / abs(truth), R.PARITY_FLOOR)
    print(f"N={N} reg: device {e_dev:.3e}, float32-terms statement {e_ref:.3e}")
    assert e_dev <= R.PARITY_FACTOR * e_ref
    assert reg4.shape == () and reg4.dtype == torch.float32
    alone = P.zero_one_loss(tx, EPS)
    assert host(alone).view(np.uint32) == host(reg4).view(np.uint32)
    flat = P.zero_one_loss(dev(x.reshape(-1)), EPS)
    assert host(flat).view(np.uint32) == host(reg4).view(np.uint32)
    (alone * 1.5).backward()
    want = R.S32.activate_backward(q, t32["scales"], t32["opacities"], None, None, None, R.F(1.5), EPS)[2]
    assert R.same_class_and_bits(host(tx.grad).reshape(-1), want)
    # another epsilon reaches the kernel: the same bound
    other = float(P.zero_one_loss(dev(x), 0.05))
    truth = float(R.S64.activate(a, q, x, 0.05)["reg"])
    e_ref = max(abs(float(R.S32.activate(a, q, x, 0.05)["reg"]) - truth) / abs(truth), R.PARITY_FLOOR)
    assert abs(other - truth) / abs(truth) <= R.PARITY_FACTOR * e_ref


def test_autograd_contract():
    N = 65
    a, q, x, g, _ = case(N)
    # under no_grad nothing is saved and nothing is differentiable
    with torch.no_grad():
        outs = P.activate(dev(a, True), dev(q, True), dev(x, True), opacity_reg=True)
        cov = P.covariance(dev(a, True), dev(q, True))
    assert all(o.grad_fn is None and not o.requires_grad for o in outs) and cov.grad_fn is None
    outs = P.activate(dev(a), dev(q), dev(x))
    assert all(o.grad_fn is None for o in outs)
    # a modified-in-place input raises at backward
    for which in range(3):
        t = [dev(a, True), dev(q, True), dev(x, True)]
        s, r, o = P.activate(*t)
        with torch.no_grad():
            t[which].add_(1.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            (s.sum() + r.sum() + o.sum()).backward()
    ta, tq = dev(a, True), dev(q, True)
    cov = P.covariance(ta, tq)
    with torch.no_grad():
        tq.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        cov.sum().backward()
    # a double backward raises
    ta, tq, tx = dev(a, True), dev(q, True), dev(x, True)
    s, r, o = P.activate(ta, tq, tx)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(s.sum(), ta, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(P.covariance(ta, tq).sum(), tq, create_graph=True)
    # a second backward of one forward raises (autograd has freed what was saved)
    s, r, o = P.activate(ta, tq, tx)
    loss = s.sum() + o.sum()
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    # N = 0: empty tensors, no launch
    e = P.activate(dev(np.zeros((0, 3)), True), dev(np.zeros((0, 4))), dev(np.zeros((0, 1))))
    assert [tuple(t.shape) for t in e] == [(0, 3), (0, 4), (0, 1)]
    e[0].sum().backward()
    assert tuple(P.covariance(dev(np.zeros((0, 3))), dev(np.zeros((0, 4)))).shape) == (0, 6)
    # opacity as [N]
    o1 = P.activate(dev(a), dev(q), dev(x.reshape(-1)))[2]
    assert tuple(o1.shape) == (N,) and np.array_equal(host(o1), host(P.activate(dev(a), dev(q), dev(x))[2]).reshape(-1))
    torch.cuda.synchronize()


def test_through_the_operator():
    """activate -> render -> backward on a small textured scene: the raw parameters' gradients are the statement's backward of the
    gradients the operator actually delivered (retain_grad), so no discrete decision of the rasterizer can enter"""
    import helpers as Hh
    from texgs import synth
    from texgs.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    N = 2000
    scene = synth.make_scene(N, 32, seed=21, scale_mean=0.05)
    cam = synth.fibonacci_cameras(4, 64, 64)[1]
    d = torch.device(DEV)
    st = Hh.settings_for(cam, 2, torch.tensor([0.1, 0.0, 0.2]), device=d, cls=GaussianRasterizationSettings)
    rng = np.random.default_rng(9)
    a = np.log(scene.scales.numpy()).astype(R.F)
    q = (scene.rotations.numpy() * rng.uniform(0.5, 2.0, (N, 1))).astype(R.F)
    x = torch.logit(scene.opacities.clamp(1e-4, 1 - 1e-4)).numpy().astype(R.F)
    ta, tq, tx = dev(a, True), dev(q, True), dev(x, True)
    s, r, o = P.activate(ta, tq, tx)
    for t in (s, r, o):
        t.retain_grad()
    t_ = lambda v: v.to(d)
    m3 = t_(scene.means3D)
    out = GaussianRasterizer(raster_settings=st)(means3D=m3, means2D=torch.zeros_like(m3), shs=t_(scene.shs), opacities=o, scales=s, rotations=r,
                                                 uvs=t_(scene.uvs), gradient_uvs=t_(scene.gradient_uvs), texture=t_(scene.texture),
                                                 extra_attrs=None)
    target, nhat = synth.make_targets(cam.image_height, cam.image_width, seed=3)
    loss = synth.synthetic_loss(out[0], out[3], out[2], target.to(d), nhat.to(d))
    before = P.BACKWARD_CALLS["activate"]
    loss.backward()
    assert P.BACKWARD_CALLS["activate"] == before + 1
    gs, gr, go = host(s.grad), host(r.grad), host(o.grad)
    assert np.abs(gs).max() > 0 and np.abs(gr).max() > 0 and np.abs(go).max() > 0
    f64, f32 = R.S64.activate(a, q, x), R.S32.activate(a, q, x)
    truth = R.S64.activate_backward(q, f64["scales"], f64["opacities"], gs, gr, go, None)
    stated = R.S32.activate_backward(q, f32["scales"], f32["opacities"], gs, gr, go, None)
    n = R.S64.norm(q.astype(np.float64))
    scales = (np.abs(truth[0]), (np.linalg.norm(gr.astype(np.float64), axis=1) / n)[:, None], np.abs(truth[2]))
    for name, t, got, tr, stt, sc in zip(("d_scaling", "d_rotation", "d_opacity"), (ta, tq, tx), (ta.grad, tq.grad, tx.grad), truth, stated, scales):
        e_dev = R.max_error(host(got), tr, sc)
        e_ref = max(R.max_error(stt, tr, sc), R.PARITY_FLOOR)
        print(f"operator {name}: device {e_dev:.3e}, float32 statement {e_ref:.3e}")
        assert e_dev <= R.PARITY_FACTOR * e_ref, name
    # a second backward raises; so does a modified-in-place input
    with pytest.raises(RuntimeError):
        loss.backward()
    s, r, o = P.activate(ta, tq, tx)
    out = GaussianRasterizer(raster_settings=st)(means3D=m3, means2D=torch.zeros_like(m3), shs=t_(scene.shs), opacities=o, scales=s, rotations=r,
                                                 uvs=t_(scene.uvs), gradient_uvs=t_(scene.gradient_uvs), texture=t_(scene.texture),
                                                 extra_attrs=None)
    with torch.no_grad():
        tq.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        out[0].sum().backward()
    torch.cuda.synchronize()
