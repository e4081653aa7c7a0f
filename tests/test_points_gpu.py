"""-m gpu: texgs.points on an MI355X against the statement in tests/points_ref.py.  The 3-NN values are compared BIT for bit and the
farthest-point index sequences for equality: a pruning rule that is not exact, a fused multiply-add or a wrong tie fails here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_bit_equal(got, want, what):
    got, want = got.detach().cpu(), torch.as_tensor(want).cpu()
    assert got.dtype == torch.float32 and want.dtype == torch.float32 and got.shape == want.shape
    same = _bits(got) == _bits(want)
    bad = int((~same).sum())
    if bad:
        i = int(torch.nonzero(~same)[0, 0])
        raise AssertionError(f"{what}: {bad} of {got.numel()} values differ; first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


@pytest.mark.parametrize("n", [4, 5, 257, 1000])
def test_knn3_small_bit_equal_numpy(n):
    from texgs import points
    p = R.clustered(n, 100 + n) if n >= 257 else R.uniform(n, 100 + n)
    _assert_bit_equal(points.knn3_mean_dist2(_dev(p)), torch.from_numpy(R.knn3_np(p)), f"N = {n}")


@pytest.fixture(scope="module")
def clustered_100k():
    p = R.clustered(100_000, 5)
    return p, R.knn3_torch(_dev(p))


def test_knn3_100k_uniform_bit_equal():
    from texgs import points
    p = R.uniform(100_000, 4)
    _assert_bit_equal(points.knn3_mean_dist2(_dev(p)), R.knn3_torch(_dev(p)), "100 000 uniform")


def test_knn3_100k_clustered_bit_equal(clustered_100k):
    from texgs import points
    p, want = clustered_100k
    _assert_bit_equal(points.knn3_mean_dist2(_dev(p)), want, "100 000 clustered")


def test_knn3_does_not_depend_on_input_order(clustered_100k):
    from texgs import points
    p, want = clustered_100k
    perm = np.random.default_rng(9).permutation(p.shape[0])
    got = points.knn3_mean_dist2(_dev(p[perm]))
    _assert_bit_equal(got, want[torch.from_numpy(perm)], "permuted 100 000 clustered")


@pytest.mark.parametrize("cloud", ["line", "plane", "identical", "one_repeated"])
def test_knn3_degenerate_clouds_bit_equal(cloud):
    from texgs import points
    p = {"line": lambda: R.on_line(3000, 1), "plane": lambda: R.on_plane(3000, 2), "identical": lambda: R.identical(1000),
         "one_repeated": lambda: R.one_repeated(300, 200, 3)}[cloud]()
    got = points.knn3_mean_dist2(_dev(p))
    _assert_bit_equal(got, torch.from_numpy(R.knn3_np(p)), cloud)
    if cloud == "identical":
        assert torch.equal(got.cpu(), torch.zeros(1000))


def test_knn3_against_float64():
    """the derived bound of test_points_host.test_fp32_statement_against_float64: 8 u = 4.8e-7 <= 1e-6"""
    from texgs import points
    p = R.clustered(20_000, 6)
    got = points.knn3_mean_dist2(_dev(p)).cpu().numpy().astype(np.float64)
    e = R.knn3_np(p, dtype=np.float64)
    zero = e == 0
    assert np.all(got[zero] == 0)
    rel = np.abs(got[~zero] - e[~zero]) / e[~zero]
    print("max relative error against float64:", float(rel.max()))
    assert float(rel.max()) <= 1e-6


def _check_fps(p, k, start, want):
    from texgs import points
    x = _dev(p)
    sel, idx = points.sample_farthest_points(x, k, start)
    assert idx.dtype == torch.int64 and idx.shape == (k,) and sel.shape == (k, 3)
    assert int(idx.min()) >= 0 and int(idx.max()) < p.shape[0]
    assert torch.equal(sel, x[idx])
    got = idx.cpu()
    if not torch.equal(got, want):
        t = int(torch.nonzero(got != want)[0, 0])
        raise AssertionError(f"FPS differs first at pick {t}: got {int(got[t])}, want {int(want[t])}")
    distinct = np.unique(p, axis=0).shape[0]
    if k <= distinct:
        assert got.unique().numel() == k


@pytest.mark.parametrize("start", [0, 613])
def test_fps_all_points_of_1000(start):
    p = R.clustered(1000, 21)
    _check_fps(p, 1000, start, torch.from_numpy(R.fps_np(p, 1000, start)))


@pytest.mark.parametrize("start", [0, 31337])
def test_fps_100k_clustered(start):
    p = R.clustered(100_000, 5)
    _check_fps(p, 2048, start, R.fps_torch(_dev(p), 2048, start))


def test_fps_k1_and_tiny():
    from texgs import points
    p = np.zeros((5, 3), dtype=np.float32)
    p[:, 0] = [0, 1, 2, 3, 10]
    assert points.sample_farthest_points(_dev(p), 5, 0)[1].tolist() == [0, 4, 3, 1, 2]
    assert points.sample_farthest_points(_dev(p), 5, 4)[1].tolist() == [4, 0, 3, 1, 2]
    assert points.sample_farthest_points(_dev(p), 1, 2)[1].tolist() == [2]


def test_extract_pcd_and_init_log_scales():
    from texgs import points
    p = R.clustered(5000, 8)
    x = _dev(p)
    assert torch.equal(points.extract_pcd(x, 5000), x)
    assert torch.equal(points.extract_pcd(x, 16384), x)
    pcd = points.extract_pcd(x, 512)
    assert pcd.shape == (512, 3) and pcd.dtype == torch.float32
    assert torch.equal(pcd, points.sample_farthest_points(x, 512, 0)[0])
    assert torch.equal(pcd.cpu(), torch.from_numpy(p[R.fps_np(p, 512, 0)]))
    ls = points.init_log_scales(x)
    assert ls.shape == (5000, 3) and ls.dtype == torch.float32 and bool(torch.isfinite(ls).all())
    want = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(R.knn3_np(p)), 0.0000001)))
    assert torch.allclose(ls[:, 0].cpu(), want, rtol=1e-6, atol=1e-6)
    assert torch.equal(ls[:, 0], ls[:, 1]) and torch.equal(ls[:, 0], ls[:, 2])
    from simple_knn._C import distCUDA2
    assert torch.equal(distCUDA2(x), points.knn3_mean_dist2(x))
    # other float dtypes are converted
    assert torch.equal(points.knn3_mean_dist2(x.double()), points.knn3_mean_dist2(x))


def test_gpu_arguments_are_checked():
    from texgs import points
    x = torch.rand(64, 3, device="cuda")
    with pytest.raises(ValueError, match="non-finite"):
        bad = x.clone()
        bad[3, 0] = float("nan")
        points.knn3_mean_dist2(bad)
    with pytest.raises(ValueError, match="K must be in"):
        points.sample_farthest_points(x, 65)
    with pytest.raises(ValueError, match="N >= 4"):
        points.knn3_mean_dist2(x[:3])


def test_stream_order_and_no_state():
    from texgs import points
    p = R.clustered(30_000, 13)
    x = _dev(p)
    first = points.knn3_mean_dist2(x)
    second = points.knn3_mean_dist2(x)
    assert torch.equal(first, second)
    f1 = points.sample_farthest_points(x, 700, 5)[1]
    f2 = points.sample_farthest_points(x, 700, 5)[1]
    assert torch.equal(f1, f2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y = _dev(p)                                  # produced on the side stream: the kernels must follow it there
        d = points.knn3_mean_dist2(y)
        idx = points.sample_farthest_points(y, 700, 5)[1]
        d_copy, idx_copy = d.clone(), idx.clone()    # read on the same stream, no synchronisation in between
    side.synchronize()
    assert torch.equal(d_copy, first) and torch.equal(idx_copy, f1)
