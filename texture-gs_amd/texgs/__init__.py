"""MI355X-native textured Gaussian rasterizer: host side of the C-ABI library libtexgs.so."""
from . import optim  # noqa: F401  (texgs.optim.FusedAdam / fused_step: the optimizer phase of a training iteration)
