"""`pytorch3d.loss.chamfer_distance` as the reference calls it: one cloud per side, no lengths, no normals, the default reductions
and squared L2, both directions or `single_directional=True`.  Every other argument value raises NotImplementedError naming it."""
from texgs import uvmap as _uvmap

_DEFAULTS = dict(x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None, batch_reduction="mean",
                 point_reduction="mean", norm=2, abs_cosine=True)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None, batch_reduction="mean",
                     point_reduction="mean", norm=2, single_directional=False, abs_cosine=True):
    """(loss, None) = texgs.uvmap.chamfer_distance(x [1, P, 3], y [1, Q, 3], single_directional)"""
    given = dict(x_lengths=x_lengths, y_lengths=y_lengths, x_normals=x_normals, y_normals=y_normals, weights=weights,
                 batch_reduction=batch_reduction, point_reduction=point_reduction, norm=norm, abs_cosine=abs_cosine)
    for k, v in given.items():
        d = _DEFAULTS[k]
        if not (v is d or (d is not None and not hasattr(v, "shape") and v == d)):
            raise NotImplementedError(f"pytorch3d drop-in: chamfer_distance({k}={v!r}) is not supported (only {k}={d!r})")
    if not isinstance(single_directional, bool):
        raise NotImplementedError(f"pytorch3d drop-in: chamfer_distance(single_directional={single_directional!r}) is not supported (a bool)")
    if hasattr(x, "dim") and x.dim() == 3 and x.shape[0] != 1:
        raise NotImplementedError(f"pytorch3d drop-in: chamfer_distance with batch size {x.shape[0]} is not supported (1)")
    return _uvmap.chamfer_distance(x, y, single_directional=single_directional)
