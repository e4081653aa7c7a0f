"""`nvdiffrast.torch.texture`, cubemap fetches only (texgs.cubetex.cube_sample; unpinned against the package, see there).

Supported: boundary_mode='cube' with tex [B, 6, R, R, C] and uv [B', ..., 3] where B == B' or B == 1, filter_mode 'auto' (which
means 'linear' here: without uv_da or mip there is nothing else for it to mean), 'linear' or 'nearest'.  Everything else raises
NotImplementedError naming the argument."""
import torch as _torch

from texgs.cubetex import cube_sample as _cube_sample

__all__ = ["texture"]


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    for name, value in (("uv_da", uv_da), ("mip_level_bias", mip_level_bias), ("mip", mip), ("max_mip_level", max_mip_level)):
        if value is not None:
            raise NotImplementedError(f"nvdiffrast.torch.texture: {name} is not supported (no mipmapped or derivative-based filtering)")
    if boundary_mode != "cube":
        raise NotImplementedError(f"nvdiffrast.torch.texture: boundary_mode={boundary_mode!r} is not supported, only 'cube'")
    if filter_mode not in ("auto", "linear", "nearest"):
        raise NotImplementedError(f"nvdiffrast.torch.texture: filter_mode={filter_mode!r} is not supported, only 'auto', 'linear' "
                                  "and 'nearest'")
    if not isinstance(tex, _torch.Tensor) or not isinstance(uv, _torch.Tensor):
        raise TypeError("nvdiffrast.torch.texture: tex and uv must be torch.Tensors")
    if tex.dim() != 5:
        raise NotImplementedError(f"nvdiffrast.torch.texture: tex must be a cubemap batch [B, 6, R, R, C], got {tuple(tex.shape)} "
                                  "(2-D textures are not supported)")
    if uv.dim() < 2 or uv.shape[-1] != 3:
        raise ValueError(f"nvdiffrast.torch.texture: uv must be [B, ..., 3] for boundary_mode='cube', got {tuple(uv.shape)}")
    if tex.shape[0] not in (1, uv.shape[0]):
        raise ValueError(f"nvdiffrast.torch.texture: tex holds {tex.shape[0]} cubemaps, uv {uv.shape[0]} batches")
    filter = "nearest" if filter_mode == "nearest" else "linear"
    if tex.shape[0] == 1:
        return _cube_sample(tex[0], uv, filter)
    return _torch.stack([_cube_sample(tex[b], uv[b], filter) for b in range(tex.shape[0])], 0)
