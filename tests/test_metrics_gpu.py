"""-m gpu: texgs.metrics (csrc/metrics.hip) against its float64 statement (tests/metrics_ref.py) and against torch's own float32
formulas on the device.

Shapes: 7x7 (one cropped pixel), 8x9, 33x65 (one pixel past a tile edge in both axes), 38x70 (a tile plus its halo), 64x64 (exact
tiles), 100x75.  Inputs (metrics_ref.image_pair): noise, a smooth sinusoid plus small noise, a nearly flat image 0.8 +- 0.005 (the
cancellation case), an identical pair, values outside [0, 1] (clamp on and off).

Bounds against the statement:
  per-channel sum S / count   1e-9 absolute.  fp64 rounding 1.1e-16 over about 100 operations, amplified by at most 1 / C2 = 1.1e3,
                              is about 1e-11; the bound is two orders above.  float32 window arithmetic sits at 4e-8 .. 8.5e-5 on
                              the flat and 7x7 cases, so a kernel that slipped back to fp32 fails there.
  sum |d|, sum d^2            1e-12 relative (the same fp32 differences, fp64 sums in another order)
  MAE                         1e-9 degrees
Against torch's float32 formulas: psnr, mse, L1 mean 1e-5 relative (fp32 eps times the reduction); mae 1e-3 degrees on normals at
least 5 degrees apart, where float32 acos is well conditioned."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_SSIM, TOL_SUM, TOL_MAE = 1e-9, 1e-12, 1e-9


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_row(got, want, what):
    """one row of the kernel against the statement's, at the module's bounds; each figure is printed before it is asserted"""
    got = np.asarray(got, np.float64)
    assert got.shape == (16,)
    e_ssim = float(np.abs(got[4:7] - want[4:7]).max() / want[10])
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if np.abs(b).max() > 0 else float(np.abs(a).max())
    e_l1, e_se = rel(got[0:1], want[0:1]), rel(got[1:4], want[1:4])
    e_mae = abs(got[7] / got[8] - want[7] / want[8]) if want[8] > 0 else 0.0
    e_den = rel(got[8:9], want[8:9])
    print(f"{what}: SSIM {e_ssim:.2e} (bound {TOL_SSIM:.0e})  sum|d| {e_l1:.2e}  sum d^2 {e_se:.2e} (bound {TOL_SUM:.0e})  "
          f"MAE {e_mae:.2e} deg (bound {TOL_MAE:.0e})")
    assert e_ssim <= TOL_SSIM, (what, e_ssim)
    assert e_l1 <= TOL_SUM and e_se <= TOL_SUM and e_den <= TOL_SUM, (what, e_l1, e_se, e_den)
    assert e_mae <= TOL_MAE, (what, e_mae)
    assert got[9] == want[9] and got[10] == want[10] and not got[11:].any(), what
    if want[8] == 0:
        assert got[7] == 0 and got[8] == 0, what


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_against_the_statement(lib_built, shape):
    """every input kind at one shape through one Evaluator: clamp off everywhere, clamp on as well for the out-of-range pair;
    normals with alpha, without alpha and absent take turns"""
    from texgs import metrics
    H, W = shape
    n1, n2, alpha = M.normal_pair(H, W, seed=1)
    views = []
    for i, kind in enumerate(M.KINDS):
        x, y = M.image_pair(kind, H, W, seed=2)
        for clamp in ((False, True) if kind == "out_of_range" else (False,)):
            nrm = (n1, n2, alpha) if i % 3 == 0 else (n1, n2, None) if i % 3 == 1 else (None, None, None)
            views.append((kind, clamp, x, y) + nrm)
    ev = metrics.Evaluator(capacity=len(views))
    for kind, clamp, x, y, a, b, al in views:
        ev.add(_dev(x), _dev(y), norm=_dev(a), gt_norm=_dev(b), alpha=_dev(al), clamp=clamp)
    rows = ev.rows().cpu().numpy()
    assert rows.shape == (len(views), 16)
    for r, (kind, clamp, x, y, a, b, al) in zip(rows, views):
        want = M.row(x, y, a, b, al, clamp=clamp)
        _assert_row(r, want, f"{H}x{W} {kind} clamp={clamp}")
        if kind == "identical":
            assert r[0] == 0 and not r[1:4].any() and np.array_equal(r[4:7], np.full(3, want[10]))      # S is exactly 1 everywhere
    on, off = rows[-1], rows[-2]
    assert abs(on[0] - off[0]) > 1e-3 * off[0]          # the clamp did something


@pytest.mark.parametrize("shape", [(7, 7), (33, 65), (100, 75)], ids=lambda s: "%dx%d" % s)
def test_functions_against_torch_float32_formulas(lib_built, shape):
    """utils/metrics.py:18-37 and losses/pixelwise_loss.py:3-4 written out in torch float32 on the device"""
    from texgs import metrics
    H, W = shape
    for kind in ("noise", "smooth", "flat"):
        x, y = (_dev(t) for t in M.image_pair(kind, H, W, seed=3))
        want_mse = ((x - y) ** 2).view(3, -1).mean(1, keepdim=True)
        want_psnr = 20 * torch.log10(1.0 / torch.sqrt(want_mse))
        want_l1 = torch.abs(x - y).mean()
        got_mse, got_psnr = metrics.mse(x, y), metrics.psnr(x, y)
        assert got_mse.shape == (3, 1) and got_psnr.shape == (3, 1) and got_mse.dtype == torch.float32 and got_mse.is_cuda
        ev = metrics.Evaluator(1)
        ev.add(x, y, clamp=False)
        res = ev.result()
        e = [float(((got_mse - want_mse).abs() / want_mse).max()), float(((got_psnr - want_psnr).abs() / want_psnr.abs()).max()),
             abs(res["l1"] - float(want_l1)) / float(want_l1), abs(res["psnr"] - float(want_psnr.mean())) / abs(float(want_psnr.mean()))]
        print(f"{H}x{W} {kind}: relative error against float32 torch: mse {e[0]:.2e} psnr {e[1]:.2e} l1 {e[2]:.2e} "
              f"mean psnr {e[3]:.2e} (bound 1e-5)")
        assert max(e) <= 1e-5, (kind, e)
        got_ssim = metrics.ssim(x, y)
        assert isinstance(got_ssim, float)
        assert abs(got_ssim - M.ssim(x.cpu().numpy(), y.cpu().numpy())) <= TOL_SSIM
        assert abs(res["ssim"] - got_ssim) <= 1e-15 and res["mae"] is None and res["views"] == 1
    x = _dev(M.image_pair("identical", H, W, seed=3)[0])
    assert bool(torch.isinf(metrics.psnr(x, x.clone())).all()) and not bool(metrics.mse(x, x.clone()).any())
    assert metrics.ssim(x, x.clone()) == 1.0


@pytest.mark.parametrize("shape", [(7, 7), (33, 65), (100, 75)], ids=lambda s: "%dx%d" % s)
def test_mae_function(lib_built, shape):
    from texgs import metrics
    H, W = shape
    n1, n2, alpha = M.normal_pair(H, W, seed=4)
    t1, t2, ta = _dev(n1), _dev(n2), _dev(alpha)
    cos = torch.clamp(torch.cosine_similarity(t1.view(3, -1), t2.view(3, -1), dim=0, eps=1e-6), -1.0 + 1e-10, 1.0 - 1e-10)
    deg = torch.acos(cos) * (180.0 / np.pi)
    for al, want32 in ((None, deg.mean()), (ta, (deg.reshape_as(ta) * ta.float()).sum() / ta.float().sum())):
        got = metrics.mae(t1, t2, al)
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        want64 = M.mae(n1, n2, None if al is None else alpha)
        e32, e64 = abs(float(got) - float(want32)), abs(float(got) - want64)
        print(f"{H}x{W} alpha={al is not None}: |mae - float32 torch| {e32:.2e} deg (bound 1e-3), |mae - statement| {e64:.2e} deg")
        assert e32 <= 1e-3
        assert e64 <= 2.0 ** -24 * want64 + TOL_MAE      # the float32 rounding of the returned tensor; the row itself is held to 1e-9 above
    assert float(metrics.mae(t1, t1.clone())) == 0.0 and float(metrics.mae(t2, t2.clone(), ta)) == 0.0     # identical: exactly 0
    assert bool(torch.isnan(metrics.mae(t1, t2, torch.zeros_like(ta))))                                     # alpha all zero: 0 / 0
    assert float(metrics.mae(t1, t2, ta > 0.5)) == pytest.approx(M.mae(n1, n2, (alpha > 0.5).astype(np.float32)), rel=1e-6)
    z = torch.zeros_like(t1)
    assert float(metrics.mae(z, t2)) == pytest.approx(90.0, abs=1e-5)                                       # zero length: cos = 0


def test_two_adds_give_bit_identical_rows_and_add_synchronises_nothing(lib_built):
    from texgs import metrics
    H, W = 100, 75
    x, y = (_dev(t) for t in M.image_pair("smooth", H, W, seed=5))
    n1, n2, alpha = (_dev(t) for t in M.normal_pair(H, W, seed=5))
    metrics.Evaluator(1).add(x, y)                      # the library is loaded before the guard
    ev = metrics.Evaluator(capacity=4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # a host synchronisation inside the calls raises
    try:
        for _ in range(3):
            ev.add(x, y, norm=n1, gt_norm=n2, alpha=alpha)
        ev.add(x, y)
        rows = ev.rows()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    r = rows.cpu().numpy().view(np.uint64)
    assert np.array_equal(r[0], r[1]) and np.array_equal(r[0], r[2])
    assert np.array_equal(r[3, :7], r[0, :7]) and not r[3, 7:9].any() and r[0, 7:9].all()
    with pytest.raises(RuntimeError, match="capacity"):
        ev.add(x, y)
    assert len(ev) == 4


def test_sync_debug_mode_sees_a_readback(lib_built):
    """The guard above does something on this build: result(), which reads the table back, raises under it."""
    from texgs import metrics
    x, y = (_dev(t) for t in M.image_pair("noise", 8, 9, seed=6))
    ev = metrics.Evaluator(1)
    ev.add(x, y)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            ev.result()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.result()["views"] == 1


def test_evaluator_over_mixed_views_equals_the_functions_averaged(lib_built):
    """5 views of mixed size and content, clamped as train.py:52,58 clamp: result() against the per-view functions on the clamped
    images, averaged on the host as train.py:67-69,90-92 average"""
    from texgs import metrics
    spec = [("noise", 33, 65, True), ("smooth", 100, 75, False), ("out_of_range", 38, 70, True), ("flat", 7, 7, False),
            ("identical", 64, 64, True)]
    ev = metrics.Evaluator(capacity=8)
    l1, ps, ss, ma = [], [], [], []
    for k, (kind, H, W, normals) in enumerate(spec):
        x, y = (_dev(t) for t in M.image_pair(kind, H, W, seed=7))
        n1, n2, alpha = (_dev(t) for t in M.normal_pair(H, W, seed=7)) if normals else (None, None, None)
        if k == 0:
            alpha = None
        ev.add(x, y, norm=n1, gt_norm=n2, alpha=alpha)             # clamp=True
        xc, yc = torch.clamp(x, 0.0, 1.0), torch.clamp(y, 0.0, 1.0)
        l1.append(float(torch.abs(xc - yc).double().mean()))
        ps.append(float(metrics.psnr(xc, yc).double().mean()))
        ss.append(metrics.ssim(xc, yc))
        if normals:
            ma.append(float(metrics.mae(n1, n2, alpha)))
    res = ev.result()
    assert res["views"] == 5 and len(ev) == 5
    assert res["l1"] == pytest.approx(np.mean(l1), rel=1e-12)
    assert res["ssim"] == pytest.approx(np.mean(ss), abs=1e-14)
    assert res["psnr"] == float("inf") and np.mean(ps) == float("inf")          # the identical pair, as in the reference
    ev2 = metrics.Evaluator(capacity=4)
    for k, (kind, H, W, normals) in enumerate(spec[:4]):
        x, y = (_dev(t) for t in M.image_pair(kind, H, W, seed=7))
        ev2.add(x, y)
    assert ev2.result()["psnr"] == pytest.approx(np.mean(ps[:4]), rel=1e-6)     # psnr() returns float32
    assert ev2.result()["mae"] is None
    assert res["mae"] == pytest.approx(np.mean(ma), rel=1e-6)                   # mae() returns float32


def test_golden_rows(lib_built):
    from texgs import metrics
    G = M.golden()
    for tag in ("noise9x11", "range12x10", "smooth33x35"):
        get = lambda k: _dev(G[f"{tag}_{k}"]) if f"{tag}_{k}" in G.files else None
        ev = metrics.Evaluator(1)
        ev.add(get("image"), get("gt"), norm=get("norm"), gt_norm=get("gt_norm"), alpha=get("alpha"), clamp=bool(G[f"{tag}_clamp"]))
        _assert_row(ev.rows()[0].cpu().numpy(), G[f"{tag}_row"], tag)


def test_rendered_view_end_to_end(lib_built):
    """The smallest synthetic scene (400 Gaussians, 96x64), rendered forward-only; image, norm and alpha go straight from the
    rasterizer into Evaluator.add, and the row is compared with the statement on the copied-back outputs."""
    import helpers as Hh
    from texgs import metrics, synth
    scene = synth.make_scene(400, 32, seed=21, scale_mean=0.05)
    cam = synth.fibonacci_cameras(4, 96, 64)[1]
    target, nhat = synth.make_targets(cam.image_height, cam.image_width, seed=3)
    with torch.no_grad():
        out, _ = Hh.hip_run(scene, cam, 2, torch.tensor([0.1, 0.0, 0.2]))
    image, norm, alpha = out[0], out[2], out[3]
    assert tuple(image.shape) == (3, 64, 96) and float(alpha.max()) > 0.5
    ev = metrics.Evaluator(capacity=1)
    ev.add(image, target.cuda(), norm=norm, gt_norm=nhat.cuda(), alpha=alpha)
    want = M.row(image.cpu().numpy(), target.numpy(), norm.cpu().numpy(), nhat.numpy(), alpha.cpu().numpy(), clamp=True)
    _assert_row(ev.rows()[0].cpu().numpy(), want, "rendered 64x96")
    res = ev.result()
    assert res["views"] == 1 and 0.0 < res["ssim"] < 1.0 and 0.0 < res["mae"] < 180.0 and np.isfinite(res["psnr"])
