"""A bias-free ReLU MLP of width 128 as ONE fused HIP kernel per direction (csrc/mlp.hip, include/texgs_mlp.h): what tiny-cuda-nn's
`Network(n_in, n_out, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128})` computes --
the reference builds four of them per model (models/modules/utils.py:18-41): 3 -> 128 -> 128, 32 -> 128 -> 128 and twice
128 -> 128 -> 128 -> 3.

    pin = pad16(n_in), pout = pad16(n_out), L = n_hidden_layers
    params = W_1 [128, pin] | L - 1 matrices [128, 128] | W_out [pout, 128]      flat fp32, row-major, no biases: the layout
                                                                                  texgs.uvnet.unpack_tcnn_params documents
    xp  = [x | 1 ... 1]            (the padded input columns are ones: their weights act as a learned first-layer bias)
    h_1 = relu(W_1 xp);  h_k = relu(W_k h_{k-1});  y = (W_out h_L)[:n_out]

* `fused_mlp(x, params, n_in, n_out, n_hidden_layers)` is differentiable w.r.t. x and params: the forward stores no activation, the
  backward recomputes them per tile of points in LDS and keeps the weight gradients in registers; it saves only x and params, runs
  only the products `needs_input_grad` asks for, and is deterministic (no atomics).  Arithmetic: f32-input MFMA, f32 accumulation.
* `FusedMLP` is the nn.Module: one flat `params` Parameter.

Supported: width 128, 1 or 2 hidden layers, 1 <= n_in, n_out <= 128; anything else raises NotImplementedError naming the value.
No CPU fallback: CPU tensors raise.  The C entry points take bare pointers, so every argument is checked here, before any launch
(tests/mlp_ref.py holds the float64 statement the tests compare against)."""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib

WIDTH = 128                         # TEXGS_MLP_WIDTH
MAX_HIDDEN_LAYERS = 2               # TEXGS_MLP_MAX_HIDDEN_LAYERS
FORWARD_TILE = 128                  # TEXGS_MLP_FORWARD_TILE: points per workgroup of the forward kernel
BACKWARD_TILE = 64                  # TEXGS_MLP_BACKWARD_TILE: points per tile of the backward kernel
BACKWARD_MAX_WORKGROUPS = 256       # TEXGS_MLP_BACKWARD_MAX_WORKGROUPS: its persistent grid
ALIGN = 16                          # input and output widths are padded to multiples of 16


class MlpStruct(C.Structure):
    """ctypes mirror of TexGSMlp (include/texgs_mlp.h), 16 bytes"""
    _fields_ = [("n_in", C.c_int32), ("n_out", C.c_int32), ("n_hidden_layers", C.c_int32), ("n_neurons", C.c_int32)]


_vp, _i32, _size = C.c_void_p, C.c_int32, C.c_size_t
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_mlp.h
SIGNATURES = {
    "texgs_mlp_param_count": (_size, [C.POINTER(MlpStruct)]),
    "texgs_mlp_forward_temp_bytes": (_size, [C.POINTER(MlpStruct), _i32]),
    "texgs_mlp_backward_temp_bytes": (_size, [C.POINTER(MlpStruct), _i32]),
    "texgs_mlp_forward": (C.c_int, [C.POINTER(MlpStruct), _vp, _vp, _i32, _vp, _vp, _vp]),
    "texgs_mlp_backward": (C.c_int, [C.POINTER(MlpStruct), _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


def pad16(k):
    return -(-int(k) // ALIGN) * ALIGN


def check_shape(n_in, n_out, n_hidden_layers, n_neurons=WIDTH):
    """The supported envelope, by name; host arithmetic only"""
    for name, v in (("n_in", n_in), ("n_out", n_out), ("n_hidden_layers", n_hidden_layers), ("n_neurons", n_neurons)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"fused_mlp: {name} must be an int, got {type(v).__name__}")
    if n_neurons != WIDTH:
        raise NotImplementedError(f"fused_mlp: n_neurons = {n_neurons} is not supported (the kernel is written for width {WIDTH})")
    if not 1 <= n_hidden_layers <= MAX_HIDDEN_LAYERS:
        raise NotImplementedError(f"fused_mlp: n_hidden_layers = {n_hidden_layers} is not supported (1 or {MAX_HIDDEN_LAYERS})")
    if not 1 <= n_in <= WIDTH:
        raise NotImplementedError(f"fused_mlp: n_in = {n_in} is not supported (1 to {WIDTH})")
    if not 1 <= n_out <= WIDTH:
        raise NotImplementedError(f"fused_mlp: n_out = {n_out} is not supported (1 to {WIDTH})")


def matrix_shapes(n_in, n_out, n_hidden_layers):
    """[(rows, cols)] of the matrices of `params`, in order"""
    check_shape(n_in, n_out, n_hidden_layers)
    return [(WIDTH, pad16(n_in))] + [(WIDTH, WIDTH)] * (n_hidden_layers - 1) + [(pad16(n_out), WIDTH)]


def param_count(n_in, n_out, n_hidden_layers):
    return sum(a * b for a, b in matrix_shapes(n_in, n_out, n_hidden_layers))


def _check_args(x, params, n_in, n_out, n_hidden_layers):
    """Everything the kernels will index, before any launch"""
    check_shape(n_in, n_out, n_hidden_layers)
    if not isinstance(x, torch.Tensor) or not isinstance(params, torch.Tensor):
        raise TypeError("fused_mlp: x and params must be torch.Tensors")
    if x.dim() != 2 or x.shape[1] != n_in:
        raise ValueError(f"fused_mlp: x must be [N, {n_in}], got {tuple(x.shape)}")
    need = param_count(n_in, n_out, n_hidden_layers)
    if params.dim() != 1 or params.numel() != need:
        raise ValueError(f"fused_mlp: expected a flat params tensor of {need} values for {n_in} -> {n_out} with {n_hidden_layers} hidden "
                         f"layer(s) of {WIDTH}, got shape {tuple(params.shape)}")
    if x.shape[0] > 2 ** 31 - 1 - FORWARD_TILE:
        raise ValueError(f"fused_mlp: x holds {x.shape[0]} rows; the library counts tiles with 32 bits")
    for name, t in (("x", x), ("params", params)):
        if t.device.type != "cuda":
            raise RuntimeError(f"fused_mlp: {name} must be on an AMD GPU; there is no CPU fallback")
    if x.device != params.device:
        raise ValueError(f"fused_mlp: x is on {x.device}, params on {params.device}")


def _f32(t):
    """detached contiguous fp32 (a non-contiguous or non-fp32 tensor is copied; a 4-byte storage offset is fine: rows are read as scalars)"""
    return t.detach().to(torch.float32).contiguous()


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, n_in, n_out, n_hidden_layers):
        _check_args(x, params, n_in, n_out, n_hidden_layers)
        lib = entry()
        xx, pp = _f32(x), _f32(params)
        N = xx.shape[0]
        y = torch.empty(N, n_out, dtype=torch.float32, device=xx.device)
        st = MlpStruct(n_in, n_out, n_hidden_layers, WIDTH)
        p = _lib.ptr
        with _lib.on(xx.device) as stream:
            temp = torch.empty(max(16, lib.texgs_mlp_forward_temp_bytes(C.byref(st), N)), dtype=torch.uint8, device=xx.device)
            _lib.call(lib.texgs_mlp_forward, C.byref(st), p(pp), p(xx), N, p(y), p(temp), stream)
        ctx.shape = (n_in, n_out, n_hidden_layers)
        ctx.save_for_backward(x, params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_p):
            return None, None, None, None, None
        n_in, n_out, L = ctx.shape
        lib = entry()
        xx, pp, gg = _f32(x), _f32(params), _f32(dy)
        N = xx.shape[0]
        if gg.shape != (N, n_out):
            raise ValueError(f"fused_mlp: the upstream gradient must be [{N}, {n_out}], got {tuple(gg.shape)}")
        dx = torch.empty_like(xx) if need_x else None
        dp = torch.empty_like(pp) if need_p else None
        st = MlpStruct(n_in, n_out, L, WIDTH)
        p = _lib.ptr
        with _lib.on(xx.device) as stream:
            temp = torch.empty(max(16, lib.texgs_mlp_backward_temp_bytes(C.byref(st), N)), dtype=torch.uint8, device=xx.device)
            _lib.call(lib.texgs_mlp_backward, C.byref(st), p(pp), p(xx), p(gg), N, p(dx), p(dp), p(temp), stream)
        if dx is not None and dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        if dp is not None and dp.dtype != params.dtype:
            dp = dp.to(params.dtype)
        return dx, dp, None, None, None


def fused_mlp(x, params, n_in, n_out, n_hidden_layers):
    """y f32[N, n_out] of x [N, n_in] through the MLP `params` describes (module docstring), on the current stream of x's device.
    Differentiable w.r.t. x and params."""
    return _FusedMLP.apply(x, params, n_in, n_out, n_hidden_layers)


class FusedMLP(nn.Module):
    """The MLP as a module with ONE flat fp32 Parameter `params` (tiny-cuda-nn's state form).  Initialised Xavier-uniform per
    matrix -- U(-b, b), b = sqrt(6 / (rows + cols)) of the padded matrix -- from a torch.Generator seeded with `seed`.  That is
    tiny-cuda-nn's RULE; the values are NOT bit-equal to what tiny-cuda-nn's own initialiser draws for the same seed."""

    def __init__(self, n_in, n_out, n_hidden_layers, seed=1337):
        super().__init__()
        shapes = matrix_shapes(n_in, n_out, n_hidden_layers)
        self.n_in, self.n_out, self.n_hidden_layers = n_in, n_out, n_hidden_layers
        gen = torch.Generator().manual_seed(int(seed))
        mats = []
        for a, b in shapes:
            bound = math.sqrt(6.0 / (a + b))
            mats.append((torch.rand(a * b, generator=gen) * 2 - 1) * bound)
        self.params = nn.Parameter(torch.cat(mats))

    def forward(self, x):
        return fused_mlp(x, self.params, self.n_in, self.n_out, self.n_hidden_layers)
