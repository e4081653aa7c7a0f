"""Drop-in for the part of `tinycudann` that Texture-GS calls (`import tinycudann as tcnn`, models/modules/utils.py:1-41): with
texture-gs_amd/ on PYTHONPATH, `tcnn.Network` is the fused HIP MLP of texgs.mlp and `tcnn.Encoding` the HIP hash grid of
texgs.uvmap, so the reference's own `UVNet` / `InvUVNet` classes import and run as written.

    tcnn.Network(n_input_dims, n_output_dims, network_config, seed=1337)
        otype "FullyFusedMLP" or "CutlassMLP", activation "ReLU", output_activation "None", n_neurons 128, n_hidden_layers 1 or 2
    tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "HashGrid", ...})
        the limits of texgs.uvmap.HashGridEncoding (4 features per level, at most 16 levels)

Both are nn.Modules whose only state is ONE flat fp32 Parameter `params`, as in tiny-cuda-nn: the reference's
`nn.Sequential(enc, mlp)` has the keys `0.params` / `1.params`, and a reference state_dict() loads with a plain load_state_dict (fp16
checkpoints are converted by load_state_dict's copy).  The flat layouts are restated from tiny-cuda-nn's published source and are
UNPINNED against the package (texgs.uvnet.unpack_tcnn_params); the first construction says so in a RuntimeWarning.

Deviation: outputs are float32 where tiny-cuda-nn returns float16; every call site of the reference applies `.float()` at once.
Anything else -- another otype, activation, width, depth or config key, `NetworkWithInputEncoding` -- raises NotImplementedError
naming it.  Initial values follow tiny-cuda-nn's rules, not its random stream.  There is no CPU fallback."""
import warnings

from texgs import mlp as _mlp
from texgs import uvmap as _uvmap

__all__ = ["Network", "Encoding", "NetworkWithInputEncoding"]

_MLP_OTYPES = ("FullyFusedMLP", "CutlassMLP")
_NETWORK_KEYS = ("otype", "activation", "output_activation", "n_neurons", "n_hidden_layers")
_ENCODING_KEYS = {"otype": None, "n_levels": "n_levels", "n_features_per_level": "n_features", "log2_hashmap_size": "log2_hashmap_size",
                  "base_resolution": "base_resolution", "per_level_scale": "per_level_scale"}
_warned = False


def _warn_unpinned():
    global _warned
    if _warned:
        return
    _warned = True
    warnings.warn("tinycudann here is the texgs drop-in: its flat `params` layouts (FullyFusedMLP matrices, HashGrid tables) are "
                  "restated from tiny-cuda-nn's published source and are UNPINNED (tiny-cuda-nn cannot be installed in the build "
                  "container, no fixture produced by it exists): check a rendered view against the reference before trusting a "
                  "checkpoint that the real package wrote.", RuntimeWarning, stacklevel=3)


def _int(name, v):
    if isinstance(v, bool) or not (isinstance(v, int) or (isinstance(v, float) and v == int(v))):
        raise NotImplementedError(f"tinycudann drop-in: {name} = {v!r} is not supported (an integer is expected)")
    return int(v)


class Network(_mlp.FusedMLP):
    """tcnn.Network: the fused bias-free ReLU MLP.  Attributes `params`, `n_input_dims`, `n_output_dims`; float32 output."""

    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337):
        cfg = dict(network_config)
        for k in cfg:
            if k not in _NETWORK_KEYS:
                raise NotImplementedError(f"tinycudann drop-in: network_config key {k!r} is not supported (known: {', '.join(_NETWORK_KEYS)})")
        otype = cfg.get("otype", "FullyFusedMLP")
        if otype not in _MLP_OTYPES:
            raise NotImplementedError(f"tinycudann drop-in: network otype {otype!r} is not supported ({' or '.join(_MLP_OTYPES)})")
        if cfg.get("activation", "ReLU") != "ReLU":
            raise NotImplementedError(f"tinycudann drop-in: activation {cfg['activation']!r} is not supported (ReLU)")
        if cfg.get("output_activation", "None") not in ("None", None):
            raise NotImplementedError(f"tinycudann drop-in: output_activation {cfg['output_activation']!r} is not supported (None)")
        n_neurons = _int("n_neurons", cfg.get("n_neurons", 128))
        depth = _int("n_hidden_layers", cfg.get("n_hidden_layers", 2))
        n_in, n_out = _int("n_input_dims", n_input_dims), _int("n_output_dims", n_output_dims)
        try:
            _mlp.check_shape(n_in, n_out, depth, n_neurons)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("fused_mlp:", "tinycudann drop-in:").replace("n_in =", "n_input_dims =")
                                      .replace("n_out =", "n_output_dims =")) from None
        super().__init__(n_in, n_out, depth, seed=seed)
        self.n_input_dims, self.n_output_dims = n_in, n_out
        _warn_unpinned()


class Encoding(_uvmap.HashGridEncoding):
    """tcnn.Encoding with otype "HashGrid": texgs.uvmap.HashGridEncoding under tiny-cuda-nn's config keys.  `n_output_dims`."""

    def __init__(self, n_input_dims=3, encoding_config=None):
        cfg = dict(encoding_config or {})
        otype = cfg.get("otype")
        if otype != "HashGrid":
            raise NotImplementedError(f"tinycudann drop-in: encoding otype {otype!r} is not supported (HashGrid)")
        for k in cfg:
            if k not in _ENCODING_KEYS:
                raise NotImplementedError(f"tinycudann drop-in: encoding_config key {k!r} is not supported "
                                          f"(known: {', '.join(_ENCODING_KEYS)})")
        if n_input_dims != 3:
            raise NotImplementedError(f"tinycudann drop-in: n_input_dims = {n_input_dims!r} is not supported for HashGrid (3)")
        grid = {_ENCODING_KEYS[k]: v for k, v in cfg.items() if k != "otype"}
        try:
            super().__init__(**grid)
        except ValueError as e:                 # the grid limits of the library (features per level, level count, ...)
            raise NotImplementedError(f"tinycudann drop-in: HashGrid {grid} is not supported: {e}") from None
        self.n_input_dims = 3
        _warn_unpinned()


def NetworkWithInputEncoding(*args, **kwargs):
    raise NotImplementedError("tinycudann drop-in: NetworkWithInputEncoding is not supported; build nn.Sequential(Encoding, Network) as "
                              "models/modules/utils.py does")
