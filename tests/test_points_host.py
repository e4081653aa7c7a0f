"""-m "not gpu": the statement of the point-cloud operations (tests/points_ref.py) in its three forms, its rounding error against
float64, cases computed by hand, the argument checks of texgs.points, the simple_knn drop-in and the v18 ABI."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_ref as R  # noqa: E402

N, K = 8192, 1024
CLOUDS = {"uniform": lambda: R.uniform(N, 11), "clustered": lambda: R.clustered(N, 12)}


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_numpy_and_torch_statements_agree_bit_for_bit(cloud):
    p = CLOUDS[cloud]()
    a = R.knn3_np(p)
    b = R.knn3_torch(torch.from_numpy(p)).numpy()
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for start in (0, 77):
        ia = R.fps_np(p, K, start)
        ib = R.fps_torch(torch.from_numpy(p), K, start).numpy()
        assert np.array_equal(ia, ib)


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_fp32_statement_against_float64(cloud):
    """Derived bound, u = 2^-24: each d2 carries <= 5u (difference u, square 2u + u, two additions of non-negative terms), the
    ordered sum two more, the division one: 8u = 4.8e-7 <= 1e-6.  A near-tie that makes fp32 pick another third neighbour moves
    the value by no more than the same bound."""
    p = CLOUDS[cloud]()
    a = R.knn3_np(p).astype(np.float64)
    e = R.knn3_np(p, dtype=np.float64)
    zero = e == 0
    assert np.all(a[zero] == 0)
    rel = np.abs(a[~zero] - e[~zero]) / e[~zero]
    print(cloud, "max relative error of the fp32 statement:", float(rel.max()), "zeros:", int(zero.sum()))
    assert float(rel.max()) <= 1e-6


def test_cube_corners_by_hand():
    # every corner has three neighbours at distance 1 (the edges); the next ones are at sqrt(2)
    assert np.array_equal(R.knn3_np(R.cube_corners()), np.ones(8, dtype=np.float32))
    assert torch.equal(R.knn3_torch(torch.from_numpy(R.cube_corners())), torch.ones(8))


def test_coincident_points_by_hand():
    p = np.array([[1, 2, 3]] * 4 + [[50, 2, 3]], dtype=np.float32)
    got = R.knn3_np(p)
    assert np.array_equal(got[:4], np.zeros(4, dtype=np.float32))         # three other copies at distance 0
    assert got[4] == np.float32(49 * 49)                                    # (2401 + 2401 + 2401) / 3
    # init_log_scales of that: clamp_min(0, 1e-7) -> log(sqrt(1e-7)), the formula of models/gaussian3d.py:63-64 on the statement
    ls = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(got), 0.0000001)))
    want = math.log(math.sqrt(1e-7))
    assert torch.allclose(ls[:4], torch.full((4,), want), rtol=1e-6, atol=0)
    assert abs(float(ls[4]) - math.log(49.0)) < 1e-6


def test_fps_collinear_by_hand():
    p = np.zeros((5, 3), dtype=np.float32)
    p[:, 0] = [0, 1, 2, 3, 10]
    # start 0: m = [0, 1, 4, 9, 100] -> 4;  m = [0, 1, 4, 9, 0] -> 3;  m = [0, 1, 1, 0, 0]: tie of indices 1 and 2 -> 1; then 2
    assert R.fps_np(p, 5, 0).tolist() == [0, 4, 3, 1, 2]
    assert R.fps_torch(torch.from_numpy(p), 5, 0).tolist() == [0, 4, 3, 1, 2]
    # start 4: m = [100, 81, 64, 49, 0] -> 0;  m = [0, 1, 4, 9, 0] -> 3;  m = [0, 1, 1, 0, 0]: tie -> 1; then 2
    assert R.fps_np(p, 5, 4).tolist() == [4, 0, 3, 1, 2]
    assert R.fps_torch(torch.from_numpy(p), 5, 4).tolist() == [4, 0, 3, 1, 2]
    assert R.fps_np(p, 1, 2).tolist() == [2]


def test_arguments_are_checked_before_any_launch(lib_built, monkeypatch):
    from texgs import _lib, points

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    ok = torch.rand(16, 3)
    for f in (points.knn3_mean_dist2, points.init_log_scales, points.extract_pcd, lambda p: points.sample_farthest_points(p, 4)):
        with pytest.raises(RuntimeError, match="points.*no CPU fallback"):
            f(ok)
        with pytest.raises(ValueError, match=r"points must be \[N, 3\]"):
            f(torch.rand(16, 2))
        with pytest.raises(ValueError, match=r"points must be \[N, 3\]"):
            f(torch.rand(16))
        with pytest.raises(ValueError, match="points holds non-finite"):
            bad = ok.clone()
            bad[5, 1] = float("nan")
            f(bad)
        with pytest.raises(ValueError, match="points holds non-finite"):
            bad = ok.clone()
            bad[0, 2] = float("inf")
            f(bad)
        with pytest.raises(ValueError, match="floating-point"):
            f(torch.zeros(16, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="points needs N >= 4"):
        points.knn3_mean_dist2(torch.rand(3, 3))
    with pytest.raises(ValueError, match="points needs N >= 4"):
        points.init_log_scales(torch.rand(3, 3))
    with pytest.raises(ValueError, match=r"K must be in \[1, N = 16\], got K = 17"):
        points.sample_farthest_points(ok, 17)
    with pytest.raises(ValueError, match=r"K must be in \[1, N = 16\], got K = 0"):
        points.sample_farthest_points(ok, 0)
    with pytest.raises(ValueError, match="start_index must be in"):
        points.sample_farthest_points(ok, 4, start_index=16)
    with pytest.raises(ValueError, match="start_index must be in"):
        points.sample_farthest_points(ok, 4, start_index=-1)
    with pytest.raises(ValueError, match="num_points must be a positive int"):
        points.extract_pcd(ok, 0)


def test_c_entry_points_refuse_bad_sizes(lib_built):
    """The C layer's own checks return an error code before any launch (no GPU is needed to see them)."""
    from texgs import _lib
    lib = _lib.load()
    assert lib.texgs_knn3_mean_dist2(None, 3, None, None, None) != 0
    assert b"n < 4" in lib.texgs_last_error()
    assert lib.texgs_farthest_points(None, 8, 9, 0, None, None, None) != 0
    assert b"k must be" in lib.texgs_last_error()
    assert lib.texgs_farthest_points(None, 8, 0, 0, None, None, None) != 0
    assert lib.texgs_farthest_points(None, 8, 2, 8, None, None, None) != 0
    assert b"start must be" in lib.texgs_last_error()
    assert lib.texgs_farthest_points(None, 8, 2, 0, None, None, None) != 0
    assert b"NULL" in lib.texgs_last_error()
    assert lib.texgs_knn3_temp_bytes(100000) >= 7 * 4 * 100000
    assert lib.texgs_fps_temp_bytes(300000, 16384) >= 4 * 300000 + 8 * 16384


def test_simple_knn_drop_in():
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    from simple_knn._C import distCUDA2
    from texgs import points
    assert distCUDA2 is points.knn3_mean_dist2
    assert points.distCUDA2 is points.knn3_mean_dist2


def test_points_does_not_import_oracle_or_tests():
    code = ("import sys; sys.path[:0]=[%r]; import texgs.points, simple_knn._C; "
            "bad = [k for k in sys.modules if k.split('.')[0] in ('oracle', 'tests', 'points_ref', 'helpers')]; "
            "assert not bad, bad" % os.path.join(ROOT, "texture-gs_amd"))
    subprocess.check_call([sys.executable, "-c", code])


def test_header_and_abi_version(lib_built):
    from texgs import _lib
    hdr = open(os.path.join(ROOT, "include", "texgs.h")).read()
    for name in ("texgs_knn3_temp_bytes", "texgs_knn3_mean_dist2", "texgs_fps_temp_bytes", "texgs_farthest_points"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+TEXGS_ABI_VERSION\s+19\b", hdr)
    assert _lib.load().texgs_abi_version() == _lib.ABI_VERSION == 19
