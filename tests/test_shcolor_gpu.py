"""-m gpu: the colour stage on the device (texgs/shcolor.py, csrc/shcolor.hip) against the numpy statements of tests/shcolor_ref.py.

The forward is compared with the float32 statement bit for bit (the statement's eval_sh half equals the reference's float32 CPU
result bit for bit: tests/test_shcolor_host.py).  For the backward the float64 statement is the truth and the float32 statement,
with the kernels' operation order, sets the bound: a field's error (max |device - float64| / scale, no element and no row
excluded) may be at most PARITY_FACTOR x the float32 statement's own, floored at 2^-24 -- the ratio rule of tests/test_params_gpu.py.

Inputs: standard-normal coefficients, points 2 to 6 units from cameras within a unit of the origin (shcolor_ref.random_case).  A
forward case is one (degree, max degree) pair over all its sizes: at N = 1 there are three entries, so the clamped share is asserted
over the pair's sizes together, and for every size from 63 rows on by itself."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shcolor_ref as R  # noqa: E402
from texgs import shcolor as S  # noqa: E402

pytestmark = pytest.mark.gpu
RPW = S.ROWS_PER_WORKGROUP
FORWARD_SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 1000]
BACKWARD_SIZES = [1, 65, RPW, RPW + 1, 4 * RPW + 1]
PAIRS = [(deg, mx) for mx in range(5) for deg in range(mx + 1)]
VIEWS = [1, 2, 3, 16, 17]
DEV = "cuda:0"


def dev(x, grad=False):
    return torch.tensor(np.asarray(x, R.F), device=DEV).requires_grad_(grad)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, R.F), np.ascontiguousarray(b, R.F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(N, K, V=1, seed=7):
    """Inputs and upstream gradients of one size: computed once, shared, never modified"""
    return R.random_case(N, K, seed + 1000 * K + N, V)


@functools.lru_cache(maxsize=None)
def statements(N, K, deg, V=1):
    """The float64 truth and the float32 statement of the backward, with the scales of the bound"""
    sh, xyz, cams, g = case(N, K, V)
    return (R.S64.colors_backward(deg, sh, xyz, cams, g), R.S32.colors_backward(deg, sh, xyz, cams, g),
            R.backward_scales(deg, sh, xyz, cams, g))


def ratios(got, N, K, deg, V=1):
    """{field: device error / float32 statement's own error} and whether the device has the statement's bits"""
    truth, stated, scales = statements(N, K, deg, V)
    out, same = {}, {}
    for name, gv, t, s, sc in zip(("d_sh", "d_xyz"), got, truth, stated, scales):
        if gv is None:
            continue
        e_dev = R.max_error(gv, t, sc)
        e_ref = max(R.max_error(s, t, sc), R.PARITY_FLOOR)
        out[name], same[name] = e_dev / e_ref, R.same_class_and_bits(gv, s)
        print(f"N={N} K={K} deg={deg} V={V} {name}: device {e_dev:.3e}, float32 statement {e_ref:.3e}, ratio {out[name]:.3f}, bits equal: {same[name]}")
    return out, same


def as_pair(sh, grad=False):
    return dev(sh[:, :1], grad), dev(sh[:, 1:], grad)


# ---- 1. forward: bit for bit ----
@pytest.mark.parametrize("deg,mx", PAIRS)
def test_forward_has_the_bits_of_the_float32_statement(deg, mx):
    K = (mx + 1) ** 2
    cols = []
    for N in FORWARD_SIZES:
        sh, xyz, cams, _ = case(N, K)
        want = R.S32.colors(deg, sh, xyz, cams[0])
        cam = dev(cams[0])
        with torch.no_grad():
            assert bits_equal(host(S.sh_colors(dev(sh), dev(xyz), cam, deg)), want), N
            assert bits_equal(host(S.sh_colors(as_pair(sh), dev(xyz), cam, deg)), want), (N, "pair")
            # eval_sh on the transposed view the reference passes, and on a contiguous [N,3,K] tensor, the statement's directions
            d = R.S32.direction(xyz, cams[0])[0] if deg else np.zeros_like(xyz)
            raw = R.S32.eval_sh(deg, sh, d)
            view = dev(sh).transpose(1, 2)
            assert not view.is_contiguous() or K == 1
            assert bits_equal(host(S.eval_sh(deg, view, dev(d))), raw), (N, "eval_sh, transposed view")
            assert bits_equal(host(S.eval_sh(deg, view.contiguous(), dev(d))), raw), (N, "eval_sh, contiguous")
            assert bits_equal(R.S32.clamp(raw), want)
        if N >= 63:
            clamped = float((want == 0).mean())
            assert (clamped >= 0.01 or deg == 0) and clamped <= 0.5, (N, clamped)
        cols.append(want.reshape(-1))
    allc = np.concatenate(cols)
    clamped = float((allc == 0).mean())
    print(f"deg={deg} K={K}: {100 * clamped:.1f} % of {allc.size} entries clamped")
    if deg >= 1:
        assert clamped >= 0.01 and 1 - clamped >= 0.5
    else:
        assert (allc == 0).any() and (allc > 0).any()


# ---- 2. backward ----
def run_backward(sh, xyz, cam, g, deg, want=(True, True), pair=False):
    tx = dev(xyz, want[1])
    if pair:
        feats = as_pair(sh, want[0])
        leaves = list(feats)
    else:
        feats = dev(sh, want[0])
        leaves = [feats]
    col = S.sh_colors(feats, tx, dev(cam), deg)
    (col * dev(g)).sum().backward()
    d_sh = None
    if want[0]:
        d_sh = np.concatenate([host(t.grad) for t in leaves], axis=1)
    return host(col), d_sh, host(tx.grad)


@pytest.mark.parametrize("deg,mx", PAIRS)
def test_backward_is_within_the_bound_at_every_size(deg, mx):
    K, A = (mx + 1) ** 2, (deg + 1) ** 2
    worst = {}
    for N in BACKWARD_SIZES:
        sh, xyz, cams, g = case(N, K)
        col, d_sh, d_xyz = run_backward(sh, xyz, cams[0], g[0], deg)
        r, same = ratios((d_sh, d_xyz), N, K, deg)
        for name, v in r.items():
            assert v <= R.PARITY_FACTOR, (N, name, v)
            worst[name] = max(worst.get(name, 0.0), v)
        assert not d_sh[:, A:].any()                                    # the inactive coefficients: exactly zero
        gate_closed = np.broadcast_to((col == 0)[:, None, :], d_sh[:, :A].shape)
        assert not d_sh[:, :A][gate_closed].any()                      # a clamped entry contributes exactly nothing
        if deg == 0:
            assert not d_xyz.any()
        # the flavours: only the features, only xyz, the pair's two outputs -- the same bits as the full call
        _, only_sh, none_xyz = run_backward(sh, xyz, cams[0], g[0], deg, want=(True, False))
        _, none_sh, only_xyz = run_backward(sh, xyz, cams[0], g[0], deg, want=(False, True))
        _, pair_sh, pair_xyz = run_backward(sh, xyz, cams[0], g[0], deg, pair=True)
        assert none_xyz is None and none_sh is None
        assert bits_equal(only_sh, d_sh) and bits_equal(only_xyz, d_xyz) and bits_equal(pair_sh, d_sh) and bits_equal(pair_xyz, d_xyz), N
        # two calls: the same bits
        _, again_sh, again_xyz = run_backward(sh, xyz, cams[0], g[0], deg)
        assert bits_equal(again_sh, d_sh) and bits_equal(again_xyz, d_xyz)
    print("PARITY", json.dumps({"deg": deg, "K": K, "worst_ratio": worst}))


def test_pair_outputs_are_optional_each():
    N, K, deg = 2 * RPW + 3, 16, 2
    sh, xyz, cams, g = case(N, K)
    full = run_backward(sh, xyz, cams[0], g[0], deg)
    for want_dc, want_rest in ((True, False), (False, True)):
        dc, rest = dev(sh[:, :1], want_dc), dev(sh[:, 1:], want_rest)
        (S.sh_colors((dc, rest), dev(xyz), dev(cams[0]), deg) * dev(g[0])).sum().backward()
        assert (dc.grad is None) == (not want_dc) and (rest.grad is None) == (not want_rest)
        if want_dc:
            assert bits_equal(host(dc.grad), full[1][:, :1])
        else:
            assert bits_equal(host(rest.grad), full[1][:, 1:])


def test_eval_sh_backward_on_both_layouts():
    N, K = RPW + 7, 25
    sh, xyz, cams, g = case(N, K)
    d = R.S32.direction(xyz, cams[0])[0]
    for deg in range(5):
        w_sh, w_dirs = R.S32.eval_sh_backward(deg, sh, d, g[0])
        t_sh, t_dirs = R.S64.eval_sh_backward(deg, sh, d, g[0])
        s_sh, s_xyz = R.backward_scales(deg, sh, xyz, cams, g)
        s_dirs = s_xyz * np.linalg.norm(xyz.astype(np.float64) - cams[0], axis=1, keepdims=True)
        for layout in ("view", "contiguous"):
            feats = dev(sh, True)
            view = feats.transpose(1, 2) if layout == "view" else feats.transpose(1, 2).contiguous()
            td = dev(d, True)
            (S.eval_sh(deg, view, td) * dev(g[0])).sum().backward()
            for name, got, truth, stated, scale in (("d_sh", host(feats.grad), t_sh, w_sh, s_sh), ("d_dirs", host(td.grad), t_dirs, w_dirs, s_dirs)):
                ratio = R.max_error(got, truth, scale) / max(R.max_error(stated, truth, scale), R.PARITY_FLOOR)
                print(f"eval_sh deg={deg} {layout} {name}: ratio {ratio:.3f}, bits equal: {R.same_class_and_bits(got, stated)}")
                assert ratio <= R.PARITY_FACTOR, (deg, layout, name, ratio)
            assert not host(feats.grad)[:, (deg + 1) ** 2:].any()


# ---- 3. views ----
@pytest.mark.parametrize("V", VIEWS)
def test_views_equal_the_single_view_calls_and_sum_in_view_order(V):
    N, K, deg = 2 * RPW + 1, 16, 3
    sh, xyz, cams, g = case(N, K, V)
    before = dict(S.CALLS)

    def run(pair=False):
        feats = as_pair(sh, True) if pair else dev(sh, True)
        tx = dev(xyz, True)
        cols = S.sh_colors_views(feats, tx, dev(cams), deg)
        (cols * dev(g)).sum().backward()
        leaves = feats if pair else [feats]
        return host(cols), np.concatenate([host(t.grad) for t in leaves], axis=1), host(tx.grad)

    cols, d_sh, d_xyz = run()
    launches = (V + S.MAX_VIEWS - 1) // S.MAX_VIEWS
    assert S.CALLS["forward"] == before["forward"] + launches and S.CALLS["backward"] == before["backward"] + launches
    assert cols.shape == (V, N, 3)
    with torch.no_grad():
        for v in range(V):
            assert bits_equal(cols[v], host(S.sh_colors(dev(sh), dev(xyz), dev(cams[v]), deg))), v
    r, same = ratios((d_sh, d_xyz), N, K, deg, V)
    print("PARITY", json.dumps({"V": V, "ratios": r, "bits_equal": same}))
    for name, v in r.items():
        assert v <= R.PARITY_FACTOR, (name, v)
    again = run()
    assert bits_equal(again[0], cols) and bits_equal(again[1], d_sh) and bits_equal(again[2], d_xyz)
    pair = run(pair=True)
    assert bits_equal(pair[0], cols) and bits_equal(pair[1], d_sh) and bits_equal(pair[2], d_xyz)


# ---- 4. special rows ----
def test_special_rows_keep_to_themselves():
    N, K = RPW + 5, 25
    sh, xyz, cams, g = (np.array(v) for v in case(N, K, 2))
    xyz[3] = cams[1]                    # a point at the second camera's centre: 0 / 0 there
    sh[7, 2, 1] = np.nan
    sh[11, 20, 0] = np.nan              # beyond degree 3: not read at degree <= 3
    for deg in range(5):
        feats, tx = dev(sh, True), dev(xyz, True)
        cols = S.sh_colors_views(feats, tx, dev(cams), deg)
        (cols * dev(g)).sum().backward()
        c = host(cols)
        want = R.S32.colors_views(deg, sh, xyz, cams)
        assert R.same_class_and_bits(c, want), deg
        nan = np.isnan(c)
        expect = np.zeros_like(nan)
        if deg >= 1:
            expect[1, 3, :] = True      # torch's class: NaN in that view only
            expect[:, 7, 1] = True
        if deg == 4:
            expect[:, 11, 0] = True
        assert np.array_equal(nan, expect), deg
        w_sh, w_xyz = R.S32.colors_backward(deg, sh, xyz, cams, g)
        d_sh, d_xyz = host(feats.grad), host(tx.grad)
        rows = np.ones(N, bool)
        rows[[3, 7, 11]] = False        # every other row: untouched by the three
        assert R.same_class_and_bits(d_sh[rows], w_sh[rows]) and R.same_class_and_bits(d_xyz[rows], w_xyz[rows])
        assert np.isfinite(d_sh[rows]).all() and np.isfinite(d_xyz[rows]).all()
        assert R.same_class_and_bits(d_sh, w_sh) and R.same_class_and_bits(d_xyz, w_xyz)       # the three: whatever the statement yields


def test_autograd_plumbing():
    N, K = 70, 16
    sh, xyz, cams, g = case(N, K)
    feats, tx, cam = dev(sh, True), dev(xyz, True), dev(cams[0]).requires_grad_(True)
    col = S.sh_colors(feats, tx, cam, 3)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad((col * dev(g[0])).sum(), feats, create_graph=True)
    col = S.sh_colors(feats, tx, cam, 3)
    (col * dev(g[0])).sum().backward()
    assert cam.grad is None                         # no gradient to the camera centre
    col = S.sh_colors(feats, tx, cam, 3)
    with torch.no_grad():
        tx.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        col.sum().backward()
    with torch.no_grad():                           # nothing saved, nothing differentiable
        assert not S.sh_colors(feats, tx, cam, 3).requires_grad
    empty = S.sh_colors(dev(np.zeros((0, K, 3))), dev(np.zeros((0, 3))), cam, 3)
    assert tuple(empty.shape) == (0, 3)
    # a side stream: the launches go to the current stream, nothing waits on the host
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        on_side = S.sh_colors(dev(sh), dev(xyz), dev(cams[0]), 3)
    side.synchronize()
    assert bits_equal(host(on_side), R.S32.colors(3, sh, xyz, cams[0]))


# ---- 5. through the rasterizer ----
def _render(kind, scene, features, cam, deg, bg, target, nhat):
    import diff_gauss as dg
    import helpers as Hh
    from texgs import synth
    d = torch.device(DEV)
    st = Hh.settings_for(cam, min(deg, 3), bg, device=d, cls=dg.GaussianRasterizationSettings)
    means = scene.means3D.float().to(d).requires_grad_(True)
    feats = features.to(d).requires_grad_(True)
    campos = cam.camera_center.float().to(d)
    if kind == "hip":
        kw = dict(colors_precomp=S.sh_colors(feats, means, campos, deg))
    elif kind == "torch":
        kw = dict(colors_precomp=R.torch_lines(feats, means, campos, deg))
    else:
        kw = dict(shs=feats)
    m2 = torch.zeros(means.shape[0], 3, device=d, requires_grad=True)
    out = dg.GaussianRasterizer(st)(means3D=means, means2D=m2, opacities=scene.opacities.float().to(d), scales=scene.scales.float().to(d),
                                    rotations=scene.rotations.float().to(d), cov3Ds_precomp=None, extra_attrs=None, **kw)
    synth.synthetic_loss(out[0], out[3], out[2], target.to(d), nhat.to(d)).backward()
    return out[0].detach().cpu(), feats.grad.cpu(), means.grad.cpu()


def test_colors_precomp_through_diff_gauss_three_ways(lib_built):
    """A small diff_gauss render with colors_precomp from this stage, from the torch lines restated in shcolor_ref.torch_lines, and with shs=: images
    within the project's 1e-4 per pixel, features.grad rows within its 1e-3 (helpers.grad_close).  At degree 4 -- a path shs= cannot
    take -- the first two."""
    import helpers as Hh
    from texgs import synth
    N = 3000
    scene = synth.make_scene(N, 8, seed=31, scale_mean=0.03)
    cam = synth.fibonacci_cameras(4, 64, 64)[1]
    bg = torch.tensor([0.1, 0.0, 0.2])
    target, nhat = synth.make_targets(64, 64, seed=5)
    gen = torch.Generator().manual_seed(12)
    for deg, K in ((3, 16), (4, 25)):
        features = torch.cat([torch.randn(N, 1, 3, generator=gen), 0.4 * torch.randn(N, K - 1, 3, generator=gen)], 1)
        img_h, gf_h, gm_h = _render("hip", scene, features, cam, deg, bg, target, nhat)
        img_t, gf_t, gm_t = _render("torch", scene, features, cam, deg, bg, target, nhat)
        print(f"deg {deg}: image hip vs torch lines {float((img_h - img_t).abs().max()):.2e}")
        assert float((img_h - img_t).abs().max()) < 1e-4, deg
        ok, msg = Hh.grad_close(gf_h, gf_t)
        assert ok, (deg, "features vs the torch lines", msg)
        ok, msg = Hh.grad_close(gm_h, gm_t)
        assert ok, (deg, "means vs the torch lines", msg)
        assert gf_h[:, 1:].abs().max() > 0
        if deg == 3:
            img_s, gf_s, _ = _render("shs", scene, features, cam, deg, bg, target, nhat)
            print(f"deg {deg}: image hip vs shs= {float((img_h - img_s).abs().max()):.2e}")
            assert float((img_h - img_s).abs().max()) < 1e-4
            ok, msg = Hh.grad_close(gf_h, gf_s)
            assert ok, ("features vs shs=", msg)
