"""The cases of the LPIPS stage's GPU checks, stated once: tests/test_lpips_gpu.py asserts on them and scripts/lpips_parity.py measures
them.  Inputs by seed, both CPU evaluations of tests/lpips_ref.py (float64 and the same loops in float32) computed once per case and
shared read-only, and the helpers that run a case on the GPU.

x and y of a convolution are VIEWS into NaN-filled buffers (`embed`): PAD NaN rows above and below and PAD NaN columns left and right
of every channel plane, and a whole NaN plane behind every image, so between batch slots too.  A tap read from outside an image -- a
row end wrapped into the next row, a row past the bottom, the next plane or the next image -- surfaces as NaN in y; a store outside
the Ho x Wo elements of a plane is seen in y's guard cells afterwards."""
import functools

import numpy as np
import torch

import lpips_ref as R

PAD = 2               # NaN rows / columns on every side of a plane (2: a 2x2 pool window that starts on the last row or column)


def conv_cases():
    from texgs import lpips as L
    th, tw, ck, ct = L.TILE_H, L.TILE_W, L.CIN_STEP, L.COUT_TILE
    c = lambda B, Cin, Cout, H, W, **kw: dict(dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, pool=False, affine=False, relu=True, zero_bias=False,
                                                   plant=False), **kw)
    return [
        c(1, 3, 64, 16, 16, affine=True), c(2, 3, 64, 17, 23, affine=True),              # K = 27 is padded; a wrong border shows the shift
        c(3, 16, 16, 1, 1), c(1, 16, 16, 2, 2, pool=True),                               # 1x1: every tap but the centre is padding
        c(2, 24, 48, 5, 37),                                                              # Cout no multiple of 64
        c(2, 64, 64, 9, tw * 2 + 1), c(1, 64, 64, th + 1, 7),                            # tiles straddle the right and the bottom edge
        c(1, 64, 128, 19, 21, pool=True, plant=True),                                    # pooled 9x10: the odd row and column are dropped
        c(1, 512, 512, 3, 3),                                                             # K = 4608: the deepest accumulation
        c(2, 24, 48, 5, 37, relu=False), c(1, 16, 16, 4, 5, zero_bias=True),
        # from the tile constants: Cin around the channel step, Cout around the tile, H and W around the pixel tile
        c(1, ck - 1, ct + 16, th - 1, tw - 1), c(1, ck + 1, ct - 16, th, tw), c(2, 2 * ck + 1, 2 * ct, 2 * th + 1, tw + 1),
        c(1, ck, ct, 2 * th + 3, 2 * tw + 3, pool=True, affine=True),                    # pooled (th + 1) x (tw + 1), affine in front of the pool
    ]


def cid(c):
    return "x".join(str(c[k]) for k in ("B", "Cin", "Cout", "H", "W")) + "".join("-" + k for k in ("pool", "affine", "plant", "zero_bias") if c[k]) \
        + ("" if c["relu"] else "-norelu")


N_CONV = 15


@functools.lru_cache(maxsize=None)
def conv_case(k):
    """Inputs and both CPU evaluations of case k, computed once and shared (read-only)"""
    c = conv_cases()[k]
    rng = np.random.default_rng(100 + k)
    x = rng.standard_normal((c["B"], c["Cin"], c["H"], c["W"])).astype(np.float32)
    if c["plant"]:                                  # the largest values sit in the row and column that the pool drops
        x[:, :, c["H"] - 1, :] = 50.0
        x[:, :, :, c["W"] - 1] = 60.0
    w = (rng.standard_normal((c["Cout"], c["Cin"], 3, 3)) * np.sqrt(2.0 / (9 * c["Cin"]))).astype(np.float32)
    b = np.zeros(c["Cout"], np.float32) if c["zero_bias"] else rng.standard_normal(c["Cout"]).astype(np.float32)
    sc = sh = None
    if c["affine"]:
        sc, sh = rng.uniform(0.5, 2.0, c["Cin"]).astype(np.float32), rng.uniform(1.0, 3.0, c["Cin"]).astype(np.float32)      # a non-zero shift
    args = (x, w, b, c["relu"], c["pool"], sc, sh)
    out = dict(x=x, w=w, b=b, sc=sc, sh=sh, y64=R.conv3x3(*args), y32=R.conv3x3(*args, fp32=True))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return c, out


def embed(a):
    """A [B, C, h, w] array, tensor or shape inside a NaN-filled GPU buffer (module docstring) -> (buffer, view); the view holds
    a copy of `a`, or NaN when only a shape was given"""
    shape = tuple(a) if isinstance(a, (tuple, list, torch.Size)) else tuple(a.shape)
    B, Cn, h, w = shape
    buf = torch.full((B, Cn + 1, h + 2 * PAD, w + 2 * PAD), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :Cn, PAD:PAD + h, PAD:PAD + w]
    if isinstance(a, np.ndarray):
        view.copy_(torch.from_numpy(np.array(a)))
    elif torch.is_tensor(a):
        view.copy_(a)
    return buf, view


def guards_intact(buf, view):
    """Every cell of `buf` outside `view` (embed's pair) is still NaN"""
    _, Cn, h, w = view.shape
    guard = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    guard[:, :Cn, PAD:PAD + h, PAD:PAD + w] = False
    return bool(torch.isnan(buf[guard]).all())


def cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def run_conv(c, d, x=None):
    """Case (c, d) on the GPU, x and y embedded; `x`: another input of the case's shape but any batch -> y (a view)"""
    from texgs import lpips as L
    _, xv = embed(d["x"] if x is None else x)
    Ho, Wo = L.out_size(c["H"], c["W"], c["pool"])
    ybuf, yv = embed((xv.shape[0], c["Cout"], Ho, Wo))
    packed = L.pack_conv3x3(cuda(d["w"]))
    L.conv3x3(xv, packed, cuda(d["b"]), relu=c["relu"], pool_in=c["pool"], in_scale=cuda(d["sc"]), in_shift=cuda(d["sh"]), out=yv)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, yv), "the kernel wrote outside y"
    return yv


# ---- the head alone ----
HEAD_CASES = [(1, 64, 1, 1, None), (3, 64, 3, 5, None), (1, 512, 37, 41, None), (3, 512, 3, 5, None), (3, 64, 37, 41, None),
              (3, 64, 3, 5, "zero-image"), (1, 512, 3, 5, "zero-pixel")]


@functools.lru_cache(maxsize=None)
def head_case(k):
    P, Cn, h, w, special = HEAD_CASES[k]
    rng = np.random.default_rng(300 + k)
    f = np.abs(rng.standard_normal((2 * P, Cn, h, w))).astype(np.float32)              # features are behind a ReLU
    f[f < 0.3] = 0.0
    if special == "zero-image":
        f[P:] = 0.0                                                                      # every feature of the partners is zero
    if special == "zero-pixel":
        f[:, :, 1, 2] = 0.0
    lin = (rng.uniform(0, 4.0 / Cn, Cn)).astype(np.float32)
    out = dict(f=f, lin=lin, v64=R.head(f[:P], f[P:], lin), v32=R.head(f[:P], f[P:], lin, fp32=True))
    for v in out.values():
        v.setflags(write=False)
    return out


def run_head(f, lin, layer=0, table=None):
    from texgs import lpips as L
    P = f.shape[0] // 2
    if table is None:
        table = torch.full((P, L.ROW), float("nan"), dtype=torch.float64, device="cuda")
    L.lpips_head(f, lin, table, layer)
    torch.cuda.synchronize()
    return table


# ---- the whole net ----
NET_SIZES = [(16, 16), (17, 31), (32, 48)]
NET_SEED = 21


@functools.lru_cache(maxsize=None)
def net():
    from texgs import lpips as L
    n = L.LPIPSVGG.random(NET_SEED)
    convs = [(w.numpy(), b.numpy()) for w, b in n.convs]
    lins = [l.numpy() for l in n.lins]
    return n, convs, lins


@functools.lru_cache(maxsize=None)
def net_case(size):
    """Two pairs of images in [0,1] and both CPU evaluations (features of the four images, the layers' terms), computed once"""
    _, convs, lins = net()
    H, W = size
    rng = np.random.default_rng(H * 100 + W)
    img0 = rng.uniform(0, 1, (2, 3, H, W)).astype(np.float32)
    img1 = np.clip(img0 + rng.normal(0, 0.15, img0.shape), 0, 1).astype(np.float32)
    x = np.concatenate([img0, img1])
    out = dict(img0=img0, img1=img1)
    for tag, fp32 in (("64", False), ("32", True)):
        taps = R.features(convs, x, normalize=True, fp32=fp32)
        out["taps" + tag] = taps
        out["layers" + tag] = np.stack([R.head(t[:2], t[2:], lin, fp32) for t, lin in zip(taps, lins)], axis=1)       # [2, 5]
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return out


def value(layers):
    v = layers[:, 0].copy()
    for k in range(1, 5):
        v = v + layers[:, k]
    return v
