"""`simple_knn._C`: the one function the reference imports from it."""
from texgs.points import knn3_mean_dist2 as distCUDA2

__all__ = ["distCUDA2"]
