"""`pytorch3d.ops.sample_farthest_points` as the reference calls it: one cloud [1, P, 3], no lengths, an int K, the walk started at
index 0 (`random_start_point=False`).  Every other argument value raises NotImplementedError naming it."""
import torch

from texgs import points as _points


def sample_farthest_points(points, lengths=None, K=50, random_start_point=False):
    """(points[:, idx] [1, K, 3], idx int64 [1, K]) from texgs.points.sample_farthest_points"""
    if lengths is not None:
        raise NotImplementedError("pytorch3d drop-in: sample_farthest_points(lengths=...) is not supported (only lengths=None)")
    if random_start_point is not False:
        raise NotImplementedError(f"pytorch3d drop-in: sample_farthest_points(random_start_point={random_start_point!r}) is not supported "
                                  "(only False: the walk starts at index 0)")
    if isinstance(K, bool) or not isinstance(K, int):
        raise NotImplementedError(f"pytorch3d drop-in: sample_farthest_points(K={K!r}) is not supported (one int for the one cloud)")
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"sample_farthest_points: points must be [1, P, 3], got {tuple(getattr(points, 'shape', ()))}")
    if points.shape[0] != 1:
        raise NotImplementedError(f"pytorch3d drop-in: sample_farthest_points with batch size {points.shape[0]} is not supported (1)")
    sampled, idx = _points.sample_farthest_points(points[0], K, 0)
    return sampled[None], idx[None]
