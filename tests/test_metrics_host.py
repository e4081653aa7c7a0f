"""-m "not gpu": the statement of the evaluation metrics (tests/metrics_ref.py) against closed forms, against the installed torch's
cosine_similarity and against tests/golden/metrics.npz; the argument checks and the host finishing of texgs.metrics; the two new
entries of the C ABI.

Bounds: closed forms of constant images 1e-12 (a handful of float64 operations on values of order 1; the constants pass through
float32, so the closed form is evaluated on the float32 values); angles 1e-9 degrees where acos is well conditioned and 2e-6
degrees at exactly orthogonal float64 inputs (exact 90 up to the last bits of pi / 2).  The golden rows are reproduced by the code
that wrote them: 1e-12 relative allows another scipy's summation order."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as M  # noqa: E402


# ---- the statement against closed forms ----
@pytest.mark.parametrize("shape", [(7, 7), (8, 9), (33, 65)])
def test_identical_images_give_ssim_exactly_one(shape):
    x, _ = M.image_pair("noise", *shape, seed=1)
    assert M.ssim(x, x.copy()) == 1.0
    assert np.isinf(M.psnr(x, x)).all() and M.l1(x, x) == 0.0


@pytest.mark.parametrize("c1, c2", [(0.25, 0.75), (0.8, 0.8), (0.0, 1.0), (0.3, 0.31)])
def test_constant_images_give_the_luminance_term(c1, c2):
    x, y = np.full((3, 11, 13), c1, np.float32), np.full((3, 11, 13), c2, np.float32)
    a, b = float(np.float32(c1)), float(np.float32(c2))
    want = (2 * a * b + M.C1) / (a * a + b * b + M.C1)
    assert abs(M.ssim(x, y) - want) <= 1e-12
    d = float(np.float32(c1) - np.float32(c2))
    assert np.allclose(M.mse(x, y), d * d, rtol=1e-14, atol=0) and abs(M.l1(x, y) - abs(d)) <= 1e-15


def test_window_larger_than_the_image_raises():
    with pytest.raises(ValueError):
        M.ssim(np.zeros((3, 6, 9), np.float32), np.zeros((3, 6, 9), np.float32))


def test_orthogonal_and_zero_length_normals_give_ninety_degrees():
    a = np.zeros((3, 2, 3), np.float32)
    b = np.zeros((3, 2, 3), np.float32)
    a[0], b[1] = 2.0, 0.5                       # x axis against y axis, neither of unit length
    assert np.abs(M.angles_deg(a, b) - 90.0).max() <= 2e-6 and abs(M.mae(a, b) - 90.0) <= 2e-6
    z = np.zeros_like(a)
    assert np.abs(M.angles_deg(z, b) - 90.0).max() <= 2e-6         # cos = 0 / (1e-6 * |b|) = 0
    assert np.abs(M.angles_deg(z, z) - 90.0).max() <= 2e-6
    assert np.abs(M.angles_deg(a, 3 * a)).max() == 0.0 and np.abs(M.angles_deg(a, -a) - 180.0).max() <= 2e-6


def test_mae_with_alpha():
    n1, n2, alpha = M.normal_pair(9, 8, seed=3)
    deg = M.angles_deg(n1, n2)
    assert deg.min() >= 5.0 - 1e-3 and deg.max() <= 60.0 + 1e-3
    a = alpha.astype(np.float64)[0]
    assert abs(M.mae(n1, n2, alpha) - (deg * a).sum() / a.sum()) <= 1e-12
    assert np.isnan(M.mae(n1, n2, np.zeros_like(alpha)))


# ---- the clamping form of torch.cosine_similarity, on tiny norms ----
def test_cosine_matches_the_installed_torch_on_tiny_norms():
    """x.y / (max(|x|, eps) max(|y|, eps)), each norm clamped on its own -- not max(|x| |y|, eps) -- which only shows when a norm is
    below eps = 1e-6.  float64 inputs, so torch's own rounding does not blur the comparison."""
    rng = np.random.RandomState(4)
    a = rng.randn(3, 64)
    b = rng.randn(3, 64)
    a[:, :16] *= 1e-7                           # |a| below eps, |b| of order 1
    b[:, 16:32] *= 3e-7                         # |b| below eps
    a[:, 32:48] *= 1e-8
    b[:, 32:48] *= 1e-9                         # both below eps
    a[:, 63] = 0.0
    got = np.cos(np.radians(M.angles_deg(a.reshape(3, 8, 8), b.reshape(3, 8, 8)))).reshape(-1)
    want = torch.cosine_similarity(torch.from_numpy(a), torch.from_numpy(b), dim=0, eps=1e-6).numpy()
    assert np.abs(want[:48]).max() < 1.0                                 # the clamp is active: not a plain cosine
    assert np.abs(got - want).max() <= 1e-12
    product_form = (a * b).sum(0) / np.maximum(np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0), 1e-6)
    assert np.abs(product_form - want)[:16].max() > 1e-3                        # the other form is told apart here


def test_mae_matches_the_reference_formula_in_float32():
    """utils/metrics.py:25-37 written out with torch in float32, on normals at least 5 degrees apart (where float32 acos is well
    conditioned): within 1e-3 degrees of the float64 statement"""
    n1, n2, alpha = M.normal_pair(16, 12, seed=2)
    t1, t2, ta = torch.from_numpy(n1), torch.from_numpy(n2), torch.from_numpy(alpha)
    cos = torch.clamp(torch.cosine_similarity(t1.view(3, -1), t2.view(3, -1), dim=0, eps=1e-6), -1.0 + 1e-10, 1.0 - 1e-10)
    deg = torch.acos(cos) * (180.0 / np.pi)
    assert abs(float(deg.mean()) - M.mae(n1, n2)) <= 1e-3
    assert abs(float((deg.reshape_as(ta) * ta).sum() / ta.sum()) - M.mae(n1, n2, alpha)) <= 1e-3


# ---- the committed fixture ----
@pytest.mark.parametrize("tag", ["noise9x11", "range12x10", "smooth33x35"])
def test_statement_reproduces_the_golden_rows(tag):
    G = M.golden()
    get = lambda k: G[f"{tag}_{k}"] if f"{tag}_{k}" in G.files else None
    r = M.row(get("image"), get("gt"), get("norm"), get("gt_norm"), get("alpha"), clamp=bool(G[f"{tag}_clamp"]))
    want = G[f"{tag}_row"]
    assert want.shape == (16,) and want.dtype == np.float64 and not want[11:].any()
    assert np.abs(r - want).max() <= 1e-12 * np.abs(want).max()
    assert want[9] == get("image").shape[1] * get("image").shape[2] and (want[7] > 0) == (get("norm") is not None)


def test_clamp_changes_the_row_of_out_of_range_values():
    G = M.golden()
    a, b = G["range12x10_image"], G["range12x10_gt"]
    assert abs(M.row(a, b, clamp=False)[0] - M.row(a, b, clamp=True)[0]) > 1.0


# ---- the C ABI ----
def test_header_declares_both_symbols_and_keeps_the_abi_version(lib_built):
    from texgs import _lib
    hdr = open(os.path.join(ROOT, "include", "texgs.h")).read()
    for name in ("texgs_eval_metrics_temp_bytes", "texgs_eval_metrics"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    m = re.search(r"#define\s+TEXGS_ABI_VERSION\s+(\d+)\b", hdr)
    assert int(m.group(1)) == 19 == _lib.ABI_VERSION == _lib.load().texgs_abi_version()
    assert re.search(r"#define\s+TEXGS_METRICS_ROW\s+%d\b" % _lib.METRICS_ROW, hdr) and _lib.METRICS_ROW == M.ROW == 16


def test_c_entry_point_refuses_bad_arguments(lib_built):
    """Checked on the host before any launch: no GPU is needed to see the error codes"""
    from texgs import _lib
    lib = _lib.load()
    for H, W in ((6, 9), (9, 6), (0, 0), (-1, 64)):
        assert lib.texgs_eval_metrics(1, 1, None, None, None, H, W, 1, 1, 1, None) != 0
        assert b"at least 7" in lib.texgs_last_error()
    for args in ((None, 1, None, None, None, 9, 9, 1, 1, 1), (1, None, None, None, None, 9, 9, 1, 1, 1),
                 (1, 1, None, None, None, 9, 9, 1, None, 1), (1, 1, None, None, None, 9, 9, 1, 1, None)):
        assert lib.texgs_eval_metrics(*args, None) != 0
        assert b"NULL" in lib.texgs_last_error()
    assert lib.texgs_eval_metrics(1, 1, 1, None, None, 9, 9, 1, 1, 1, None) != 0
    assert b"both NULL or both set" in lib.texgs_last_error()
    assert lib.texgs_eval_metrics(1, 1, None, 1, None, 9, 9, 1, 1, 1, None) != 0
    # one tile -> 9 doubles; 33 x 65 -> 2 x 3 tiles
    assert lib.texgs_eval_metrics_temp_bytes(7, 7) == 72 and lib.texgs_eval_metrics_temp_bytes(33, 65) == 6 * 72
    assert lib.texgs_eval_metrics_temp_bytes(0, 5) == 0


# ---- texgs.metrics on the host ----
def test_arguments_are_checked_before_any_library_call(lib_built, monkeypatch):
    from texgs import _lib, metrics

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    img = lambda *s, **k: torch.zeros(*s, **k)
    ev = metrics.Evaluator(capacity=2)
    for H, W in ((6, 9), (9, 6)):
        with pytest.raises(ValueError, match="at least 7"):
            ev.add(img(3, H, W), img(3, H, W))
        with pytest.raises(ValueError, match="at least 7"):
            metrics.ssim(img(3, H, W), img(3, H, W))
        with pytest.raises(ValueError, match="at least 7"):
            metrics.psnr(img(3, H, W), img(3, H, W))
    with pytest.raises(ValueError, match=r"must both be \[3,H,W\]"):
        ev.add(img(4, 9, 9), img(4, 9, 9))                              # wrong channel count
    with pytest.raises(ValueError, match=r"must both be \[3,H,W\]"):
        ev.add(img(3, 9, 9), img(3, 9, 10))
    with pytest.raises(ValueError, match=r"must both be \[3,H,W\]"):
        metrics.mse(img(9, 9), img(9, 9))
    with pytest.raises(ValueError, match="image must be contiguous"):
        ev.add(img(3, 9, 18)[:, :, ::2], img(3, 9, 9))
    with pytest.raises(ValueError, match="gt_image must be contiguous"):
        ev.add(img(3, 9, 9), img(9, 9, 3).permute(2, 0, 1))
    with pytest.raises(ValueError, match="image must be torch.float32"):
        ev.add(img(3, 9, 9, dtype=torch.float64), img(3, 9, 9, dtype=torch.float64))
    with pytest.raises(ValueError, match="gt_image must be torch.float32"):
        ev.add(img(3, 9, 9), img(3, 9, 9, dtype=torch.float16))
    with pytest.raises(ValueError, match="given together"):
        ev.add(img(3, 9, 9), img(3, 9, 9), norm=img(3, 9, 9))
    with pytest.raises(ValueError, match="given together"):
        ev.add(img(3, 9, 9), img(3, 9, 9), gt_norm=img(3, 9, 9))
    with pytest.raises(ValueError, match=r"norm must be \[3,9,9\]"):
        ev.add(img(3, 9, 9), img(3, 9, 9), norm=img(3, 9, 8), gt_norm=img(3, 9, 9))
    with pytest.raises(ValueError, match="gt_norm must be torch.float32"):
        ev.add(img(3, 9, 9), img(3, 9, 9), norm=img(3, 9, 9), gt_norm=img(3, 9, 9, dtype=torch.float64))
    with pytest.raises(ValueError, match="alpha has shape"):
        ev.add(img(3, 9, 9), img(3, 9, 9), norm=img(3, 9, 9), gt_norm=img(3, 9, 9), alpha=img(1, 9, 8))
    with pytest.raises(ValueError, match="needs norm and gt_norm"):
        ev.add(img(3, 9, 9), img(3, 9, 9), alpha=img(1, 9, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a well-formed view on the CPU
        ev.add(img(3, 9, 9), img(3, 9, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.mae(img(3, 9, 9), img(3, 9, 9))
    assert len(ev) == 0 and ev.rows().shape == (0, 16)
    with pytest.raises(ValueError, match="capacity"):
        metrics.Evaluator(capacity=0)


def test_host_finishing_from_a_hand_written_table():
    from texgs import metrics
    rows = np.zeros((3, 16))
    # view 0: 10 x 10, |d| = 0.1 everywhere; view 1: 20 x 10 with unequal channels; view 2: an identical pair
    rows[0, [0, 1, 2, 3, 4, 5, 6, 9, 10]] = [30.0, 1.0, 1.0, 1.0, 8.0, 12.0, 16.0, 100, 16]
    rows[1, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]] = [60.0, 2.0, 0.02, 0.0002, 56.0, 28.0, 14.0, 450.0, 15.0, 200, 56]
    rows[2, [4, 5, 6, 9, 10]] = [16.0, 16.0, 16.0, 100, 16]
    res = metrics.finish_rows(rows[:2], [False, True])
    assert res["views"] == 2
    assert res["l1"] == pytest.approx((0.1 + 0.1) / 2, rel=1e-15)
    # PSNR per channel, then over channels, then over views: mse 1e-2 -> 20 dB; mse 1e-2, 1e-4, 1e-6 -> 20, 40, 60 dB
    assert res["psnr"] == pytest.approx((20.0 + (20.0 + 40.0 + 60.0) / 3) / 2, rel=1e-14)
    assert res["ssim"] == pytest.approx(((0.5 + 0.75 + 1.0) / 3 + (1.0 + 0.5 + 0.25) / 3) / 2, rel=1e-15)
    assert res["mae"] == pytest.approx(30.0, rel=1e-15)                 # of the one view that had normals
    assert metrics.finish_rows(rows[:1], [False])["mae"] is None
    res = metrics.finish_rows(rows, [False, True, False])
    assert res["views"] == 3 and res["psnr"] == float("inf") and res["l1"] == pytest.approx(0.2 / 3, rel=1e-15)
    rows[1, 7] = rows[1, 8] = 0.0                                       # alpha all zero: 0 / 0
    assert np.isnan(metrics.finish_rows(rows, [False, True, False])["mae"])
    assert metrics.finish_rows(np.zeros((0, 16)), []) == dict(views=0, l1=None, psnr=None, ssim=None, mae=None)
    with pytest.raises(ValueError, match="has_norm holds"):
        metrics.finish_rows(rows, [True])


def test_avg_error_is_the_reference_formula():
    from texgs import metrics
    want = float(np.exp(np.mean(np.log([10 ** (-0.1 * 30.0), np.sqrt(1 - 0.9), 0.1]))))
    assert metrics.avg_error(30.0, 0.9, 0.1) == pytest.approx(want, rel=1e-14)
