"""LPIPS-VGG (utils/metrics.py:49-58 of the reference: `LPIPS(net="vgg")(img1, img2, normalize=True)`) on the device, in HIP
(csrc/lpips.hip, include/texgs_lpips.h): thirteen 3x3 convolutions as implicit GEMMs on the matrix cores, the 2x2 max-pools and the
input scaling folded into the load of the convolution behind them, and one head launch per tapped layer.

    net = LPIPSVGG(vgg_state, lin_state)          # two state dicts (or paths): torchvision's VGG16 and the lpips package's `vgg.pth`
    net(img0, img1, normalize=True)               # f32 [P,1,1,1] on the device, nothing is read back
    net.layers(img0, img1)                        # f64 [P,5]: the five layers' terms
    net.features(x)                               # the five tapped maps (tests, debugging)

No weight file is part of this project and none is fetched: the user hands in the two published state dicts.  The ARCHITECTURE is
restated from the published source of lpips 0.1 and is UNPINNED against the real package, which cannot be imported here (loading
says so once, as texgs.uvnet.load_reference_state does):
  * scaling layer (x - shift) / scale with shift (-.030, -.088, -.188), scale (.458, .448, .450); `normalize=True` maps [0,1] to
    [-1,1] first.  Both are ONE per-channel affine, applied while the first convolution loads its tile -- not folded into its
    weights, which would be wrong on the border: the zero padding lives behind the affine.
  * VGG16 `features` 0..29: conv-relu pairs at 0,2 | 5,7 | 10,12,14 | 17,19,21 | 24,26,28 with a 2x2 max-pool in front of slices
    2-5; taps at relu1_2, relu2_2, relu3_3, relu4_3, relu5_3.
  * per layer: unit-normalise both maps over channels (eps 1e-10 added to the norm), squared difference, 1x1 `lin` weights, mean
    over pixels; the value is the sum of the five terms.

Memory: both images run as one batch of 2P; the head of a slice runs as soon as the slice is done, so no tapped map is kept and two
ping-pong activation buffers, each as large as the largest map (`activation_floats`: 2P x 64 x H x W floats), are all there is -- about 0.33 GB each for one 800x800 pair, about 0.98 GB at
1600x1200.

Precision: "fp32" -- f32-input MFMA, exact f32 products in a k-ordered f32 chain.  "bf16x3" (TEXGS_LPIPS_BF16X3) is reserved and
refused by name: it is not built.

Backward: calling the net with grad mode on and an image that requires grad returns a value that is differentiable in the images
(texgs/lpips_grad.py, csrc/lpips_grad.hip): the same launches and the same bits as the no-grad call, but the thirteen post-ReLU maps
are kept for the backward (`grad_activation_floats`: 345.6 M floats, 1.38 GB, for one 800x800 pair) instead of two ping-pong buffers.
The backward runs the thirteen data gradients through the same convolution kernel over transposed weights and returns f32 gradients
of img0 and img1 (None for one that does not require grad; with one of them the convolutions run over P images, not 2P).  It runs
once per forward, a double backward raises, and the weights are constants.  `table`, `layers`, `features`, texgs.metrics.lpips and
Evaluator never take this path: they detach.  No CPU fallback: CPU tensors raise.  Every argument is checked here, before any library call (tests/lpips_ref.py holds the float64 statement)."""
import ctypes as C
import math
import warnings

import torch

from . import _lib

TILE_H, TILE_W = 8, 32              # TEXGS_CONV_TILE_H / _W: output pixels of one workgroup
CIN_STEP = 8                        # TEXGS_CONV_CIN_STEP: input channels staged at a time
K_STEP = 72                         # TEXGS_CONV_K_STEP = 9 CIN_STEP: K = 9 Cin is padded to a multiple of it
COUT_TILE = 64                      # TEXGS_CONV_COUT_TILE
MAX_CHANNELS = 512                  # TEXGS_CONV_MAX_CHANNELS
MAX_BATCH = 65535                   # TEXGS_CONV_MAX_BATCH
MAX_TILES = 2 ** 24                 # pixel tiles of one image: the launch's limit (include/texgs_lpips.h)
ROW = 8                             # TEXGS_LPIPS_ROW: 0-4 the layers' terms, 5 their sum, 6-7 reserved
LAYERS = 5                          # TEXGS_LPIPS_LAYERS
HEAD_MAX_BLOCKS = 1024              # TEXGS_LPIPS_HEAD_MAX_BLOCKS
PRECISION = {"fp32": 0, "bf16x3": 1}          # TEXGS_LPIPS_FP32 / _BF16X3 (the latter is refused: not built)

WIDTHS = (64, 128, 256, 512, 512)
SLICES = (2, 2, 3, 3, 3)                                    # convolutions per slice
VGG_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision's vgg16().features
SLICE_OF_INDEX = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 16                       # four pools must leave a pixel


class Conv3x3Struct(C.Structure):
    """ctypes mirror of TexGSConv3x3 (include/texgs_lpips.h)"""
    _fields_ = [("x", C.c_void_p), ("packed", C.c_void_p), ("bias", C.c_void_p), ("in_scale", C.c_void_p), ("in_shift", C.c_void_p),
                ("y", C.c_void_p), ("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("relu", C.c_int32), ("pool_in", C.c_int32), ("precision", C.c_int32),
                ("x_row", C.c_int64), ("x_chan", C.c_int64), ("x_img", C.c_int64),          # strides in floats; 0, 0, 0: dense
                ("y_row", C.c_int64), ("y_chan", C.c_int64), ("y_img", C.c_int64)]


class LpipsHeadStruct(C.Structure):
    """ctypes mirror of TexGSLpipsHead (include/texgs_lpips.h)"""
    _fields_ = [("f", C.c_void_p), ("lin", C.c_void_p), ("out", C.c_void_p), ("temp", C.c_void_p), ("P", C.c_int32), ("C", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("layer", C.c_int32)]


_vp, _i32, _size = C.c_void_p, C.c_int32, C.c_size_t
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_lpips.h
SIGNATURES = {
    "texgs_conv3x3_packed_bytes": (_size, [_i32, _i32, _i32]),
    "texgs_conv3x3_pack": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "texgs_conv3x3": (C.c_int, [C.POINTER(Conv3x3Struct), _vp]),
    "texgs_lpips_head_temp_bytes": (_size, [_i32, _i32, _i32]),
    "texgs_lpips_head": (C.c_int, [C.POINTER(LpipsHeadStruct), _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


def _precision(precision):
    if precision not in PRECISION:
        raise ValueError(f"precision must be one of {sorted(PRECISION)}, got {precision!r}")
    if precision == "bf16x3":
        raise NotImplementedError("precision 'bf16x3' (TEXGS_LPIPS_BF16X3) is not built into this library: use 'fp32'")
    return PRECISION[precision]


# ------------------------------------------------------------------------------------------------ the two kernels, one call each
def _is_plane_view(t):
    """A [B, C, h, w] view whose columns are adjacent and whose rows, planes and images do not overlap: what the strides of
    TexGSConv3x3 can describe"""
    B, Cn, h, w = t.shape
    si, sc, sr, sx = t.stride()
    return sx == 1 and sr >= w and sc >= h * sr and si >= Cn * sc


def _check_gpu_f32(name, t, shape_text, ok, views=False):
    if not torch.is_tensor(t) or not ok(t):
        raise ValueError(f"{name} must be {shape_text}, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous() and not (views and _is_plane_view(t)):
        raise ValueError(f"{name} must be contiguous" + (" or a view with adjacent columns and ascending, non-overlapping strides" if views else ""))
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on an AMD GPU; there is no CPU fallback")


def check_channels(Cin, Cout):
    if not 1 <= Cin <= MAX_CHANNELS:
        raise ValueError(f"Cin must be in [1,{MAX_CHANNELS}], got {Cin}")
    if Cout % 16 or not 16 <= Cout <= MAX_CHANNELS:
        raise ValueError(f"Cout must be a multiple of 16 in [16,{MAX_CHANNELS}], got {Cout}")


def pack_conv3x3(w, precision="fp32"):
    """w f32 [Cout, Cin, 3, 3] on the GPU -> the packed weights (a uint8 tensor) that `conv3x3` takes; once per weight set"""
    prec = _precision(precision)
    _check_gpu_f32("w", w, "[Cout, Cin, 3, 3]", lambda t: t.dim() == 4 and tuple(t.shape[2:]) == (3, 3))
    Cout, Cin = int(w.shape[0]), int(w.shape[1])
    check_channels(Cin, Cout)
    lib = entry()
    packed = torch.empty(lib.texgs_conv3x3_packed_bytes(Cin, Cout, prec), dtype=torch.uint8, device=w.device)
    with _lib.on(w.device) as stream:
        _lib.call(lib.texgs_conv3x3_pack, w.data_ptr(), Cin, Cout, prec, packed.data_ptr(), stream)
    return packed


def out_size(H, W, pool_in):
    return (H // 2, W // 2) if pool_in else (H, W)


def _strides(t):
    """(row, chan, img) of a [B, C, h, w] tensor for TexGSConv3x3: zeros for a dense one"""
    return (0, 0, 0) if t.is_contiguous() else (t.stride(2), t.stride(1), t.stride(0))


def _conv(lib, stream, x_ptr, packed, bias, in_scale, in_shift, y_ptr, B, Cin, Cout, H, W, relu, pool_in, prec, x_strides=(0, 0, 0),
          y_strides=(0, 0, 0)):
    st = Conv3x3Struct(x_ptr, packed.data_ptr(), bias.data_ptr(), _lib.ptr(in_scale), _lib.ptr(in_shift), y_ptr, B, Cin, Cout, H, W,
                       1 if relu else 0, 1 if pool_in else 0, prec, *x_strides, *y_strides)
    _lib.call(lib.texgs_conv3x3, C.byref(st), stream)


def conv3x3(x, packed, bias, relu=True, pool_in=False, in_scale=None, in_shift=None, precision="fp32", out=None):
    """y f32 [B, Cout, Ho, Wo] = act(conv3x3(pad1(in(x))) + bias) in ONE launch on the current stream (include/texgs_lpips.h has the
    definition).  `packed` = pack_conv3x3(w) for a w of [len(bias), x.shape[1], 3, 3].  x and `out` may be views into larger buffers
    (adjacent columns, rows / planes / images ascending and not overlapping): nothing outside their elements is read or written."""
    prec = _precision(precision)
    _check_gpu_f32("x", x, "[B, Cin, H, W]", lambda t: t.dim() == 4, views=True)
    _check_gpu_f32("bias", bias, "[Cout]", lambda t: t.dim() == 1)
    B, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(bias.shape[0])
    check_channels(Cin, Cout)
    if (in_scale is None) != (in_shift is None):
        raise ValueError("in_scale and in_shift must be given together")
    for name, t in (("in_scale", in_scale), ("in_shift", in_shift)):
        if t is not None:
            _check_gpu_f32(name, t, f"[{Cin}]", lambda t: tuple(t.shape) == (Cin,))
    Ho, Wo = out_size(H, W, pool_in)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"x of {H}x{W} leaves no pixel behind the pool")
    if not 1 <= B <= MAX_BATCH or B * Ho * Wo >= 2 ** 31:
        raise ValueError(f"the batch must be in [1,{MAX_BATCH}] with B Ho Wo below 2^31, got B = {B}, {Ho}x{Wo}")
    if -(-Ho // TILE_H) * -(-Wo // TILE_W) >= MAX_TILES:
        raise ValueError(f"an image must have fewer than 2^24 tiles of {TILE_H}x{TILE_W} output pixels, got {Ho}x{Wo}")
    lib = entry()
    need = lib.texgs_conv3x3_packed_bytes(Cin, Cout, prec)
    if not torch.is_tensor(packed) or packed.dtype != torch.uint8 or packed.numel() != need or packed.device != x.device:
        raise ValueError(f"packed must be pack_conv3x3 of a [{Cout}, {Cin}, 3, 3] weight on {x.device} ({need} bytes)")
    for name, t in (("bias", bias), ("in_scale", in_scale), ("in_shift", in_shift)):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name} is on {t.device}, x on {x.device}")
    if out is None:
        out = torch.empty(B, Cout, Ho, Wo, dtype=torch.float32, device=x.device)
    else:
        _check_gpu_f32("out", out, f"[{B}, {Cout}, {Ho}, {Wo}]", lambda t: tuple(t.shape) == (B, Cout, Ho, Wo), views=True)
        if out.device != x.device:
            raise ValueError(f"out is on {out.device}, x on {x.device}")
    with _lib.on(x.device) as stream:
        _conv(lib, stream, x.data_ptr(), packed, bias, in_scale, in_shift, out.data_ptr(), B, Cin, Cout, H, W, relu, pool_in, prec,
              _strides(x), _strides(out))
    return out


def _head(lib, stream, f_ptr, lin, table, P, Cn, h, w, layer):
    temp = torch.empty(max(8, lib.texgs_lpips_head_temp_bytes(P, h, w)) // 8, dtype=torch.float64, device=table.device)
    st = LpipsHeadStruct(f_ptr, lin.data_ptr(), table.data_ptr(), temp.data_ptr(), P, Cn, h, w, layer)
    _lib.call(lib.texgs_lpips_head, C.byref(st), stream)


def lpips_head(f, lin, table, layer):
    """One tapped layer: f f32 [2P, C, h, w] (first images, then their partners), lin f32 [C] -> column `layer` of the caller's
    f64 [P, 8] `table` (and column 5, the sum of columns 0-4, when layer == 4).  Enqueues on the current stream; returns table."""
    _check_gpu_f32("f", f, "[2P, C, h, w]", lambda t: t.dim() == 4 and t.shape[0] >= 2 and t.shape[0] % 2 == 0)
    P, Cn, h, w = int(f.shape[0]) // 2, int(f.shape[1]), int(f.shape[2]), int(f.shape[3])
    _check_gpu_f32("lin", lin, f"[{Cn}]", lambda t: tuple(t.shape) == (Cn,))
    if not 1 <= Cn <= MAX_CHANNELS or h < 1 or w < 1 or h * w >= 2 ** 31 or P > MAX_BATCH:
        raise ValueError(f"f of {tuple(f.shape)} is outside the head's limits (C <= {MAX_CHANNELS}, h w < 2^31, P <= {MAX_BATCH})")
    if not torch.is_tensor(table) or table.dtype != torch.float64 or tuple(table.shape) != (P, ROW) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous float64 [{P}, {ROW}]")
    if not 0 <= int(layer) < LAYERS:
        raise ValueError(f"layer must be in [0,{LAYERS - 1}], got {layer}")
    if lin.device != f.device or table.device != f.device:
        raise ValueError(f"f is on {f.device}, lin on {lin.device}, table on {table.device}")
    lib = entry()
    with _lib.on(f.device) as stream:
        _head(lib, stream, f.data_ptr(), lin, table, P, Cn, h, w, int(layer))
    return table


# ------------------------------------------------------------------------------------------------ the weights
def _load_state(state, what):
    if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__"):
        state = torch.load(state, map_location="cpu", weights_only=True)
    if not hasattr(state, "keys"):
        raise TypeError(f"{what} must be a state dict or a path to one, got {type(state).__name__}")
    return state


def vgg_tensors(vgg_state, widths=WIDTHS):
    """The thirteen (weight, bias) pairs from either naming: torchvision's `features.{i}.weight` or the lpips package's
    `net.slice{s}.{i}.weight`.  A missing entry raises KeyError, a mis-shaped one ValueError, both naming the key."""
    out, cin = [], 3
    couts = [c for c, n in zip(widths, SLICES) for _ in range(n)]
    for i, s, cout in zip(VGG_INDICES, SLICE_OF_INDEX, couts):
        pair = []
        for leaf, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            names = (f"features.{i}.{leaf}", f"net.slice{s}.{i}.{leaf}")
            key = next((k for k in names if k in vgg_state), None)
            if key is None:
                raise KeyError(f"the VGG state dict has neither {names[0]!r} nor {names[1]!r}")
            t = vgg_state[key]
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"{key!r} must be a tensor of shape {shape}, got {tuple(getattr(t, 'shape', ()))}")
            pair.append(t.detach().to(torch.float32).contiguous())
        out.append(tuple(pair))
        cin = cout
    return out


def lin_tensors(lin_state, widths=WIDTHS):
    """The five `lin` weight vectors [C] from `lin{k}.model.1.weight` ([1, C, 1, 1]); a `lins.{k}.` prefix is accepted too"""
    out = []
    for k, c in enumerate(widths):
        names = (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight")
        key = next((n for n in names if n in lin_state), None)
        if key is None:
            raise KeyError(f"the lin state dict has neither {names[0]!r} nor {names[1]!r}")
        t = lin_state[key]
        if not torch.is_tensor(t) or tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"{key!r} must be a tensor of shape {(1, c, 1, 1)}, got {tuple(getattr(t, 'shape', ()))}")
        out.append(t.detach().to(torch.float32).reshape(c).contiguous())
    return out


def input_affine(normalize):
    """(in_scale, in_shift) f32 [3] of the first convolution: the scaling layer, behind [0,1] -> [-1,1] when `normalize`.
    x -> ((2x - 1) - shift) / scale = x (2 / scale) + (-1 - shift) / scale."""
    shift, scale = torch.tensor(SHIFT, dtype=torch.float64), torch.tensor(SCALE, dtype=torch.float64)
    if normalize:
        return (2.0 / scale).to(torch.float32), ((-1.0 - shift) / scale).to(torch.float32)
    return (1.0 / scale).to(torch.float32), (-shift / scale).to(torch.float32)


def activation_floats(B, H, W, widths=WIDTHS):
    """Floats of ONE of the two ping-pong activation buffers for B images of H x W: the largest map any convolution writes.  Slice
    s writes widths[s] channels at (H >> s) x (W >> s); for VGG16's widths that is slice 0's, but a width tuple may grow faster
    than the pools shrink the map."""
    need, h, w = 0, int(H), int(W)
    for s, c in enumerate(widths):
        if s > 0:
            h, w = out_size(h, w, True)
        need = max(need, int(B) * int(c) * h * w)
    return need


def grad_activation_floats(P, H, W, widths=WIDTHS):
    """Floats of the thirteen post-ReLU maps that a differentiable call keeps until its backward, for P pairs of H x W: every
    convolution of slice s writes 2P x widths[s] x (H >> s) x (W >> s).  345.6 M floats (1.38 GB) for one 800x800 pair."""
    need, h, w = 0, int(H), int(W)
    for s, (c, n) in enumerate(zip(widths, SLICES)):
        if s > 0:
            h, w = out_size(h, w, True)
        need += n * 2 * int(P) * int(c) * h * w
    return need


def _check_images(img0, img1):
    """Everything a launch relies on, before any library call -> (img0, img1 as [P,3,H,W], unbatched)"""
    for name, t in (("img0", img0), ("img1", img1)):
        if not torch.is_tensor(t) or t.dim() not in (3, 4) or t.shape[-3] != 3:
            raise ValueError(f"{name} must be [3,H,W] or [P,3,H,W], got {tuple(getattr(t, 'shape', ()))}")
    if img0.shape != img1.shape:
        raise ValueError(f"img0 and img1 must have one shape, got {tuple(img0.shape)} and {tuple(img1.shape)}")
    H, W = int(img0.shape[-2]), int(img0.shape[-1])
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"H and W must be at least {MIN_SIZE} (four 2x2 pools must leave a pixel), got {H}x{W}")
    for name, t in (("img0", img0), ("img1", img1)):
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if img0.dim() == 4 and not 1 <= img0.shape[0] <= MAX_BATCH // 2:
        raise ValueError(f"the number of pairs must be in [1,{MAX_BATCH // 2}], got {img0.shape[0]}")
    for name, t in (("img0", img0), ("img1", img1)):
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} must be on an AMD GPU; texgs.lpips has no CPU fallback")
    if img0.device != img1.device:
        raise ValueError(f"img0 is on {img0.device}, img1 on {img1.device}")
    unbatched = img0.dim() == 3
    img0, img1 = img0.detach(), img1.detach()
    return (img0[None], img1[None], True) if unbatched else (img0, img1, False)


class LPIPSVGG:
    """The metric as an object (module docstring).  Not an nn.Module: it has no parameters to train; it is differentiable in the
    images only."""

    def __init__(self, vgg_state, lin_state, precision="fp32", widths=WIDTHS, _warn=True):
        _precision(precision)
        self.precision = precision
        self.widths = tuple(int(c) for c in widths)
        if len(self.widths) != LAYERS:
            raise ValueError(f"widths must hold {LAYERS} channel counts")
        for c in self.widths:
            check_channels(c, c)
        self.convs = vgg_tensors(_load_state(vgg_state, "vgg_state"), self.widths)      # host copies: [(w, b)] x 13
        self.lins = lin_tensors(_load_state(lin_state, "lin_state"), self.widths)       # [lin] x 5
        self._device = {}                                                               # (device, precision) -> packed weights
        self._device_grad = {}                                                          # likewise, the data gradients' (transposed)
        if _warn:
            warnings.warn("LPIPSVGG restates the architecture of lpips 0.1 (scaling layer, taps, pools, head) from its published "
                          "source; it is UNPINNED against the real package, which cannot be imported here", RuntimeWarning, stacklevel=2)

    @classmethod
    def random(cls, seed, widths=WIDTHS, precision="fp32"):
        """He-scaled random convolution weights (std = sqrt(2 / (9 Cin))), small biases, non-negative lin weights, from a
        torch.Generator seeded with `seed`: what the tests and the benchmark use.  No warning: nothing of the package is claimed."""
        gen = torch.Generator().manual_seed(int(seed))
        vgg, lin, cin = {}, {}, 3
        couts = [c for c, n in zip(widths, SLICES) for _ in range(n)]
        for i, cout in zip(VGG_INDICES, couts):
            vgg[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))
            vgg[f"features.{i}.bias"] = torch.randn(cout, generator=gen) * 0.05
            cin = cout
        for k, c in enumerate(widths):
            lin[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=gen) / c * 4.0
        return cls(vgg, lin, precision=precision, widths=widths, _warn=False)

    # (the drop-in's surface: a metric object has nothing to move or to switch)
    def to(self, *args, **kwargs):
        return self

    def eval(self):
        return self

    def cuda(self, *args, **kwargs):
        return self

    def _weights(self, device):
        """The packed weights on `device`, packed once per (device, precision)"""
        key = (device, self.precision)
        w = self._device.get(key)
        if w is None:
            convs = []
            for wt, b in self.convs:
                convs.append((pack_conv3x3(wt.to(device), self.precision), b.to(device), int(wt.shape[1]), int(wt.shape[0])))
            w = dict(convs=convs, lins=[l.to(device) for l in self.lins],
                     affine={n: tuple(t.to(device) for t in input_affine(n)) for n in (False, True)})
            self._device[key] = w
        return w

    def _run(self, x, normalize, table=None, keep=False, keep_all=False):
        """x f32 [B,3,H,W] through the thirteen convolutions on the current stream.  With `table` (f64 [B/2, 8]) the head of a slice
        runs as soon as the slice is done; with `keep` the five tapped maps are cloned and returned.  With `keep_all` every
        convolution writes a buffer of its own instead of the two ping-pong ones and the thirteen maps are returned: the same
        launches, so the same bits."""
        lib = entry()
        dev = x.device
        wts = self._weights(dev)
        prec = PRECISION[self.precision]
        B, _, H, W = (int(v) for v in x.shape)
        if B * H * W >= 2 ** 31:
            raise ValueError(f"{B} images of {H}x{W} hold 2^31 pixels or more")
        scale, shift = wts["affine"][bool(normalize)]
        bufs = [] if keep_all else [torch.empty(activation_floats(B, H, W, self.widths), dtype=torch.float32, device=dev) for _ in range(2)]
        taps, maps = [], []
        with _lib.on(dev) as stream:
            src_ptr, cur, h, w, k = x.data_ptr(), 0, H, W, 0
            for s, n in enumerate(SLICES):
                for j in range(n):
                    packed, bias, cin, cout = wts["convs"][k]
                    pool = s > 0 and j == 0
                    if keep_all:
                        ho, wo = out_size(h, w, pool)
                        dst = torch.empty(B, cout, ho, wo, dtype=torch.float32, device=dev)
                        maps.append(dst)
                    else:
                        dst = bufs[cur]
                    _conv(lib, stream, src_ptr, packed, bias, scale if k == 0 else None, shift if k == 0 else None, dst.data_ptr(),
                          B, cin, cout, h, w, True, pool, prec)
                    h, w = out_size(h, w, pool)
                    src_ptr, cur, k = dst.data_ptr(), 1 - cur, k + 1
                if table is not None:
                    _head(lib, stream, src_ptr, wts["lins"][s], table, B // 2, self.widths[s], h, w, s)
                if keep:
                    taps.append(dst.view(-1)[:B * self.widths[s] * h * w].view(B, self.widths[s], h, w).clone())
        return maps if keep_all else taps

    def table(self, img0, img1, normalize=False, out=None):
        """The raw rows f64 [P, 8] on the device (columns 0-4 the layers' terms, 5 their sum); `out`: a caller-owned [P, 8] slice"""
        img0, img1, _ = _check_images(img0, img1)
        P = int(img0.shape[0])
        if out is None:
            out = torch.zeros(P, ROW, dtype=torch.float64, device=img0.device)
        elif not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (P, ROW) or not out.is_contiguous() \
                or out.device != img0.device:
            raise ValueError(f"out must be a contiguous float64 [{P}, {ROW}] on {img0.device}")
        self._run(torch.cat([img0, img1]), normalize, table=out)
        return out

    def layers(self, img0, img1, normalize=False):
        """f64 [P, 5]: the five layers' terms, on the device"""
        return self.table(img0, img1, normalize)[:, :LAYERS]

    def features(self, x, normalize=False):
        """The five tapped maps of x ([3,H,W] or [B,3,H,W]), f32 on the device (tests and debugging: each is a copy)"""
        if torch.is_tensor(x) and x.dim() == 3:
            x = x[None]
        x, _, _ = _check_images(x, x)
        return self._run(x, normalize, keep=True)

    # ---- the differentiable path (texgs/lpips_grad.py) ----
    def _grad_weights(self, device):
        """The data gradients' weights on `device`: per convolution (packed transposed weights, a zero bias, channels in, channels
        out), packed once per (device, precision)"""
        from . import lpips_grad as G
        key = (device, self.precision)
        w = self._device_grad.get(key)
        if w is None:
            w = []
            for wt, _ in self.convs:
                t = G.transposed_weight(wt).to(device)
                w.append((pack_conv3x3(t, self.precision), torch.zeros(t.shape[0], dtype=torch.float32, device=device), int(t.shape[1]),
                          int(t.shape[0])))
            self._device_grad[key] = w
        return w

    def _forward_grad(self, img0, img1, normalize):
        """The value as __call__ returns it, by the same launches, and what the backward needs: the thirteen post-ReLU maps"""
        img0, img1, unbatched = _check_images(img0, img1)
        P, _, H, W = (int(v) for v in img0.shape)
        table = torch.zeros(P, ROW, dtype=torch.float64, device=img0.device)
        maps = self._run(torch.cat([img0, img1]), normalize, table=table, keep_all=True)
        state = dict(maps=maps, P=P, H=H, W=W, normalize=bool(normalize), unbatched=unbatched, device=img0.device)
        return table[:, LAYERS].to(torch.float32).view(-1, 1, 1, 1), state

    def _backward_grad(self, state, gbar, wrt):
        """(d img0, d img1) f32 from `state` (of _forward_grad), gbar f32 [P] and wrt (1: img0, 2: img1, 3: both); None for an image
        that `wrt` leaves out.  Per slice, last first: the head's backward writes the gradient at the tapped convolution's
        output; then, per convolution, its data gradient (conv3x3 over the transposed weights) and the gate of the convolution in
        front -- or, at the head of a slice, the hand-over to the next head's backward, which routes it through the pool."""
        from . import lpips_grad as G
        wrt = G.check_wrt(wrt)
        lib, glib = entry(), G.entry()
        dev, P, H, W, maps = state["device"], state["P"], state["H"], state["W"], state["maps"]
        if maps is None:
            raise RuntimeError("LPIPSVGG: this forward's activations were consumed by an earlier backward")
        if not torch.is_tensor(gbar) or tuple(gbar.shape) != (P,) or gbar.dtype != torch.float32 or not gbar.is_contiguous() \
                or gbar.device != dev:
            raise ValueError(f"gbar must be a contiguous float32 [{P}] on {dev}")
        state["maps"] = None
        wts, gw = self._weights(dev), self._grad_weights(dev)
        prec = PRECISION[self.precision]
        Bg = G.selected(P, wrt)
        sizes = [(H, W)]
        for _ in range(1, LAYERS):
            sizes.append(out_size(*sizes[-1], True))
        new = lambda c, h, w: torch.empty(Bg * c * h * w, dtype=torch.float32, device=dev)
        with _lib.on(dev) as stream:
            k, g_next = len(maps) - 1, None
            for s in reversed(range(LAYERS)):
                (h, w), Cn = sizes[s], self.widths[s]
                grad = new(Cn, h, w)
                G._head_backward(glib, stream, maps[k].data_ptr(), wts["lins"][s], gbar, _lib.ptr(g_next), grad.data_ptr(), P, Cn, h, w, wrt)
                for j in reversed(range(SLICES[s])):
                    packed, zero, cin, cout = gw[k]
                    gin = new(cout, h, w)
                    _conv(lib, stream, grad.data_ptr(), packed, zero, None, None, gin.data_ptr(), Bg, cin, cout, h, w, False, False, prec)
                    if j > 0:                   # the partners' half of a kept map starts P images in
                        y_ptr = maps[k - 1].data_ptr() + (4 * P * cout * h * w if wrt == G.WRT_PARTNER else 0)
                        G._gate(glib, stream, gin.data_ptr(), y_ptr, Bg * cout * h * w)
                        grad = gin
                    else:
                        g_next = gin
                    maps[k] = None
                    k -= 1
            scale = wts["affine"][state["normalize"]][0]
            d = g_next.view(Bg, -1, H, W)[:, :3] * scale.view(1, 3, 1, 1)
        d0 = d[:P] if wrt & G.WRT_FIRST else None
        d1 = (d[P:] if wrt == 3 else d) if wrt & G.WRT_PARTNER else None
        if state["unbatched"]:
            d0, d1 = (None if t is None else t[0] for t in (d0, d1))
        return d0, d1

    def __call__(self, img0, img1, normalize=False):
        """f32 [P,1,1,1] ([1,1,1,1] for unbatched input: the package's shape), on the device; nothing is read back.  With grad mode
        on and an image that requires grad the value is differentiable in the images (module docstring)."""
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (img0, img1)):
            from . import lpips_grad as G
            return G.LpipsFunction.apply(img0, img1, self, bool(normalize))
        return self.table(img0, img1, normalize)[:, LAYERS].to(torch.float32).view(-1, 1, 1, 1)

    forward = __call__
