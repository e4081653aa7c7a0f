"""Point clouds between the stages of Texture-GS, without simple_knn or pytorch3d (csrc/points.hip).

* `knn3_mean_dist2` (= `distCUDA2`): mean squared distance of every point to its three nearest other points -- what stage 1
  initialises the Gaussians' scales from (models/gaussian3d.py:63-64); `init_log_scales` is those two lines.
* `sample_farthest_points`: pytorch3d.ops.sample_farthest_points for one cloud with `random_start_point=False`;
  `extract_pcd` is extract_pcd.py:17-20, the `pcd` array stage 2's chamfer loss reads.

Both are exact: the squared distance is `(dx*dx + dy*dy) + dz*dz` in fp32 without FMA, the 3-NN value is a set property and the
sampled index sequence takes the lowest index on ties (tests/points_ref.py holds the statement).  The search restates simple_knn's
published algorithm and pytorch3d's documented behaviour; both are UNPINNED against the packages.

No CPU fallback: the kernels raise on CPU tensors.  The C entry points take bare pointers, so every argument is checked here,
before any launch.
"""
import torch

from . import _lib


def _check_points(points, what):
    """-> detached contiguous fp32 [N, 3] on the GPU, all finite (one reduction and one sync: these calls run once per run)"""
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{what}: points must be a torch.Tensor, got {type(points).__name__}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be [N, 3], got {tuple(points.shape)}")
    if not points.is_floating_point():
        raise ValueError(f"{what}: points must be a floating-point tensor, got {points.dtype}")
    if points.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: points holds {points.shape[0]} rows; the library indexes them with 32 bits")
    p = points.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(p).all()):       # (a NaN would poison the Morton order silently)
        raise ValueError(f"{what}: points holds non-finite coordinates (NaN or inf)")
    if points.device.type != "cuda":
        raise RuntimeError(f"{what}: points must be on an AMD GPU; there is no CPU fallback")
    return p


def knn3_mean_dist2(points):
    """float32 [N]: ((b0 + b1) + b2) / 3 over the three smallest squared distances b0 <= b1 <= b2 from each point to the OTHER
    points (excluded by index: a duplicate contributes 0).  N >= 4."""
    if isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[0] < 4:
        raise ValueError(f"knn3_mean_dist2: points needs N >= 4 rows for three nearest other points, got N = {points.shape[0]}")
    p = _check_points(points, "knn3_mean_dist2")
    lib = _lib.load()
    n = p.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=p.device)
    with _lib.on(p.device) as stream:
        temp = torch.empty(lib.texgs_knn3_temp_bytes(n), dtype=torch.uint8, device=p.device)
        _lib.call(lib.texgs_knn3_mean_dist2, p.data_ptr(), n, out.data_ptr(), temp.data_ptr(), stream)
    return out


distCUDA2 = knn3_mean_dist2


def sample_farthest_points(points, K, start_index=0):
    """(points[idx] [K, 3], idx int64 [K]): idx[0] = start_index, then K - 1 times the point farthest from those picked so far
    (largest squared distance to its nearest pick), the lowest index on ties."""
    if isinstance(points, torch.Tensor) and points.dim() == 2:
        n = points.shape[0]
        if isinstance(K, bool) or not isinstance(K, int):
            raise TypeError(f"sample_farthest_points: K must be an int, got {type(K).__name__}")
        if isinstance(start_index, bool) or not isinstance(start_index, int):
            raise TypeError(f"sample_farthest_points: start_index must be an int, got {type(start_index).__name__}")
        if not 1 <= K <= n:
            raise ValueError(f"sample_farthest_points: K must be in [1, N = {n}], got K = {K}")
        if not 0 <= start_index < n:
            raise ValueError(f"sample_farthest_points: start_index must be in [0, N = {n}), got start_index = {start_index}")
    p = _check_points(points, "sample_farthest_points")
    lib = _lib.load()
    n = p.shape[0]
    idx = torch.empty(K, dtype=torch.int32, device=p.device)
    with _lib.on(p.device) as stream:
        temp = torch.empty(lib.texgs_fps_temp_bytes(n, K), dtype=torch.uint8, device=p.device)
        _lib.call(lib.texgs_farthest_points, p.data_ptr(), n, K, start_index, idx.data_ptr(), temp.data_ptr(), stream)
    idx = idx.long()
    return points[idx], idx


def init_log_scales(points):
    """float32 [N, 3], models/gaussian3d.py:63-64: log(sqrt(clamp_min(distCUDA2(points), 1e-7))) repeated over the three axes."""
    dist2 = torch.clamp_min(knn3_mean_dist2(points), 0.0000001)
    return torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)


def extract_pcd(xyz, num_points=16384):
    """float32 [min(N, num_points), 3], extract_pcd.py:17-20: all points when N <= num_points, else the farthest-point sample that
    starts at index 0."""
    if isinstance(num_points, bool) or not isinstance(num_points, int) or num_points < 1:
        raise ValueError(f"extract_pcd: num_points must be a positive int, got {num_points!r}")
    p = _check_points(xyz, "extract_pcd")
    if p.shape[0] <= num_points:
        return p
    return sample_farthest_points(p, num_points, 0)[0]
