"""TEST INFRASTRUCTURE ONLY -- K6 (k_render_fwd) and K7 (k_render_bwd + the texture-gradient bin reduce) on their own against float64.

A case is a record table [N,24] in the R_* layout of csrc/common.h (the names of preprocess_ref.FIELDS), a point list with per-tile
ranges, a texture [6,R,R,3] or none, an image size, a background and the four upstream gradients -- all float32 values, promoted to
float64 here, so that the device and this file see identical numbers and no rounding precedes the kernel under test.

* blend(): the forward from SURVEY A.4 per pixel, front to back, over EVERY list entry (no cull: thr / rcull are never read), and the
  backward by torch autograd only.  The per-pair intermediates (power, den, num, uv, the colour argument, the per-pair depth / normal
  features) keep their gradients; the 28 moment sums of common.h are formed from them by their definitions, each with the sum of the
  absolute values of its terms and the number of terms.  dL/dtexture is autograd on the texture leaf, likewise with sum|terms|.
* cull_aids(): thr / rcull of the device records from K1's formula in float64, rounded up to fp32.
* decision_gaps(): the relative distance of every discrete decision of every reached pair from its threshold.
* builders, one per structural edge; each nudges the offending Gaussians until every gap holds, and asserts that together with the
  floors of the edge it was built for (a case that does not reach its edge is a builder bug, not a pass)."""
import functools
import json
import math
import os
from types import SimpleNamespace

import torch

import preprocess_ref as PR

F64, F32 = torch.float64, torch.float32
TILE = 16
REC, ACC = PR.REC, PR.ACC
ALPHA_MAX, ALPHA_MIN, T_EPS, DEN_MIN, MA_MIN, SH_C0 = 0.99, 1.0 / 255.0, 1e-4, 0.2, 1e-20, 0.28209479177387814
GAP = 1e-4                         # relative distance every discrete decision keeps from its threshold
FLOOR = 8.0 * 2.0 ** -24           # a handful of fp32 roundings
EPS32 = 2.0 ** -24
MOMENT_NAMES = (["P", "Pdx", "Pdy", "Pdxdx", "Pdxdy", "Pdydy", "den", "den_dpx", "den_dpy"]
                + [f"dn{c}{s}" for c in range(3) for s in ("", "_dpx", "_dpy")]
                + ["phi0", "phi1", "phi2", "vd0", "vd1", "vd2", "depth", "n0", "n1", "n2"])
UV_SLOTS = slice(PR.M_DEN, PR.M_VD)       # M_DEN, M_DN, M_PHI: the slots an untextured blend leaves exactly 0
IMAGES = ("color", "depth", "norm", "alpha", "final_T")


class Windows:
    """A texture of nominal resolution R of which only one window per face exists: face f owns the texels [y0, y0 + h) x [x0, x0 + w),
    a dense [h, w, 3] block.  The blocks live one behind the other in `data` [sum h w, 3] (the autograd leaf); whatever blend() returns
    per texel (d_tex, d_tex_abs, d_tex_ext, d_tex_x [sum h w, 3], d_tex_n [sum h w]) has that shape, and face() cuts one window out of
    it.  index() turns (face, row, column) into rows of `data`; a tap that the caller needs and that lies outside its face's window
    is an assertion failure, never a silent zero."""

    def __init__(self, R, origins, blocks):
        self.R = int(R)
        self.y0, self.x0 = torch.tensor([int(o[0]) for o in origins]), torch.tensor([int(o[1]) for o in origins])
        self.h, self.w = torch.tensor([int(b.shape[0]) for b in blocks]), torch.tensor([int(b.shape[1]) for b in blocks])
        assert len(blocks) == 6 and all(b.dim() == 3 and b.shape[2] == 3 for b in blocks)
        self.off = torch.cumsum(self.h * self.w, 0) - self.h * self.w
        self.data = torch.cat([b.reshape(-1, 3) for b in blocks], 0).contiguous()

    def _like(self, data):
        o = Windows.__new__(Windows)
        o.__dict__.update(self.__dict__)
        o.data = data
        return o

    def to(self, dtype):
        return self._like(self.data.to(dtype))

    def clone(self):
        return self._like(self.data.clone())

    def requires_grad_(self, flag=True):
        self.data.requires_grad_(flag)
        return self

    def shifted(self, face, dy, dx):
        """the same blocks, the window of `face` moved by (dy, dx) texels: every tap of that face reads a neighbour's value"""
        o = self._like(self.data)
        o.y0, o.x0 = self.y0.clone(), self.x0.clone()
        o.y0[face] += dy
        o.x0[face] += dx
        return o

    def index(self, face, yy, xx, need):
        ly, lx = yy - self.y0[face], xx - self.x0[face]
        inside = (ly >= 0) & (ly < self.h[face]) & (lx >= 0) & (lx < self.w[face])
        assert bool(inside[need].all()), ("a tap outside its face's window", int((need & ~inside).sum()))
        z = torch.zeros_like(ly)
        return self.off[face] + torch.where(inside, ly, z) * self.w[face] + torch.where(inside, lx, z)      # (an unneeded tap: the window's first texel, weight 0)

    def face(self, per_texel, f):
        """window f of a per-texel tensor shaped like `data` -> [h, w, ...]"""
        o, h, w = int(self.off[f]), int(self.h[f]), int(self.w[f])
        return per_texel[o:o + h * w].reshape(h, w, *per_texel.shape[1:])

    @staticmethod
    def of(texture, origins, sizes):
        """the windows [y0, y0 + h) x [x0, x0 + w) of a dense [6,R,R,3] texture"""
        return Windows(texture.shape[1], origins, [texture[f, y:y + h, x:x + w] for f, ((y, x), (h, w)) in enumerate(zip(origins, sizes))])


def _texels(texture):
    """the tensor that holds a texture's values: the [6,R,R,3] tensor itself, or a Windows' data"""
    return texture.data if isinstance(texture, Windows) else texture


def _tap_index(texture, face, yy, xx, need):
    """the index of taps (face, yy, xx) into _texels(texture) and into everything shaped like it; need: the pairs whose tap is read"""
    return (texture.index(face, yy, xx, need),) if isinstance(texture, Windows) else (face, yy, xx)


class Case:
    """rec [N,24] f32; point_list int64 [D]; ranges int64 [T,2]; texture f32 [6,R,R,3], a Windows or None; bg f32 [3]; up: the four upstream
    gradients (f32, [3,H,W] / [1,H,W]); counters: the reached-edge counters of the builder."""

    def __init__(self, name, W, H, rec, point_list, ranges, texture, seed):
        self.name, self.W, self.H = name, W, H
        self.rec, self.point_list, self.ranges, self.texture = rec.to(F32).contiguous(), point_list.to(torch.int64), ranges.to(torch.int64), texture
        self.gx, self.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        assert self.ranges.shape == (self.gx * self.gy, 2)
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: (2.0 * torch.rand(*s, generator=g) - 1.0).to(F32)
        self.up = {"color": r(3, H, W), "depth": 0.3 * r(1, H, W), "norm": r(3, H, W), "alpha": r(1, H, W)}
        self.bg = torch.tensor([0.25, 0.5, 0.75], dtype=F32)
        self.counters, self.design = {}, {}

    @property
    def N(self):
        return self.rec.shape[0]

    @property
    def R(self):
        return 4 if self.texture is None else (self.texture.R if isinstance(self.texture, Windows) else self.texture.shape[1])

    def in_lists(self):
        m = torch.zeros(self.N, dtype=torch.bool)
        m[self.point_list] = True
        return m


def pre_from_rec(rec):
    """the dict preprocess_ref.record64 / cotangent_from_moments read, from a record table"""
    N = rec.shape[0]
    return dict(xy=rec[:, 0:2], conic=rec[:, 2:5], opacity=rec[:, 5], g=rec[:, 6:8], G=rec[:, 8:14].reshape(N, 3, 2), phi=rec[:, 14:17],
                viewdep=rec[:, 17:20], depth=rec[:, 20], normal=rec[:, 21:24])


# ------------------------------------------------------------------------------------------------------- float64 statement
def cube_address(uv, R):
    """direction [...,3] -> face (+x,-x,+y,-y,+z,-z: the largest |component|, ties x, y, z), in-face (col, row) in texels with texel
    centres at (i + 0.5) / R, and the margin of the face choice (largest - second largest) / largest"""
    x, y, z = uv[..., 0], uv[..., 1], uv[..., 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    ma = torch.where(isx, ax, torch.where(isy, ay, az)).clamp_min(MA_MIN)
    sc = torch.where(isx, torch.where(x >= 0, -z, z), torch.where(isy, x, torch.where(z >= 0, x, -x)))
    tc = torch.where(isx, -y, torch.where(isy, torch.where(y >= 0, z, -z), -y))
    neg = torch.where(isx, x < 0, torch.where(isy, y < 0, z < 0)).to(torch.int64)
    face = torch.where(isx, 0, torch.where(isy, 2, 4)) + neg
    col = (sc / ma + 1.0) * (0.5 * R) - 0.5
    row = (tc / ma + 1.0) * (0.5 * R) - 0.5
    srt = torch.sort(torch.stack([ax, ay, az], -1).detach(), dim=-1).values
    return face, col, row, (srt[..., 2] - srt[..., 1]) / srt[..., 2].clamp_min(MA_MIN)


def _tile_pixels(case, tile):
    ly, lx = torch.meshgrid(torch.arange(TILE), torch.arange(TILE), indexing="ij")
    py, px = ((tile // case.gx) * TILE + ly).reshape(-1), ((tile % case.gx) * TILE + lx).reshape(-1)
    block = ((lx >= 8).to(torch.int64) + 2 * (ly >= 8).to(torch.int64)).reshape(-1)
    quad = (((lx % 8) >= 4).to(torch.int64) + 2 * ((ly % 8) >= 4).to(torch.int64)).reshape(-1)
    return px, py, (px < case.W) & (py < case.H), block, quad


def _tile_forward(case, tile, rec, texture, dtype):
    """One tile, every pixel against every list entry.  -> namespace of [P,K] / [P,K,3] tensors (autograd graph attached)."""
    r0, r1 = int(case.ranges[tile, 0]), int(case.ranges[tile, 1])
    ids = case.point_list[r0:r1]
    K = ids.numel()
    px, py, inside, block, quad = _tile_pixels(case, tile)
    P = px.numel()
    pix = torch.stack([px, py], 1).to(dtype)
    t = SimpleNamespace(ids=ids, K=K, px=px, py=py, inside=inside, block=block, quad=quad)
    r = rec[ids]
    d = r[None, :, 0:2] - pix[:, None, :]                                   # dx = xy - pixel
    t.dx, t.dy = d[..., 0], d[..., 1]
    t.power = -0.5 * r[None, :, 2] * t.dx * t.dx - r[None, :, 3] * t.dx * t.dy - 0.5 * r[None, :, 4] * t.dy * t.dy
    t.power_scale = (0.5 * r[None, :, 2].abs() * t.dx * t.dx + r[None, :, 3].abs() * (t.dx * t.dy).abs()
                     + 0.5 * r[None, :, 4].abs() * t.dy * t.dy).detach()
    t.araw = r[None, :, 5] * torch.exp(t.power)
    t.alpha = t.araw + (t.araw.clamp(max=ALPHA_MAX) - t.araw).detach()    # straight-through clamp (lineage)
    with torch.no_grad():
        ok = (t.power <= 0) & (t.alpha >= ALPHA_MIN) & inside[:, None]
        Tafter = torch.cumprod(1.0 - torch.where(ok, t.alpha, torch.zeros_like(t.alpha)), 1)
        alive = Tafter >= T_EPS                                            # monotone: only a contributor candidate lowers T
        t.reached = inside[:, None] & torch.cat([torch.ones(P, 1, dtype=torch.bool), alive[:, :-1]], 1)
        t.ok, t.Tafter = ok & t.reached, Tafter
        t.contrib = ok & alive                                             # the stopping instance does not contribute
        kidx = torch.arange(1, K + 1)[None, :].expand(P, K)
        t.n_contrib = torch.where(t.contrib, kidx, torch.zeros_like(kidx)).max(1).values if K else torch.zeros(P, dtype=torch.int64)
    keep = torch.where(t.contrib, 1.0 - t.alpha, torch.ones_like(t.alpha))
    Tc = torch.cumprod(keep, 1)
    Tbefore = torch.cat([torch.ones(P, 1, dtype=dtype), Tc[:, :-1]], 1)
    t.w = torch.where(t.contrib, t.alpha * Tbefore, torch.zeros_like(t.alpha))
    t.Tfin = Tc[:, -1] if K else torch.ones(P, dtype=dtype)
    t.dpx, t.dpy = -t.dx, -t.dy                                            # dp = pixel - xy
    if texture is not None:
        R = case.R
        t.den = 1.0 + r[None, :, 6] * t.dpx + r[None, :, 7] * t.dpy
        G = r[:, 8:14].reshape(K, 3, 2)
        t.num = G[None, :, :, 0] * t.dpx[..., None] + G[None, :, :, 1] * t.dpy[..., None]
        t.good = t.den.detach() >= DEN_MIN
        den_s = torch.where(t.good, t.den, torch.ones_like(t.den))
        t.uv = r[None, :, 14:17] + torch.where(t.good[..., None], t.num / den_s[..., None], torch.zeros_like(t.num))
        t.face, t.col, t.row, t.face_margin = cube_address(t.uv, R)
        x0, y0 = torch.floor(t.col.detach()), torch.floor(t.row.detach())
        t.x0, t.y0 = x0.to(torch.int64), y0.to(torch.int64)
        # a footprint clamped at the face border reads one texel twice along that axis: the sample does not depend on the fraction
        # there, stated as such (autograd would form 0 as the difference of two equal products)
        xcl, ycl = (t.x0 < 0) | (t.x0 >= R - 1), (t.y0 < 0) | (t.y0 >= R - 1)
        t.fx = torch.where(xcl, (t.col - x0).detach(), t.col - x0)
        t.fy = torch.where(ycl, (t.row - y0).detach(), t.row - y0)
        cl = lambda v: v.clamp(0, R - 1)
        t.taps = [(cl(t.y0), cl(t.x0), (1 - t.fx) * (1 - t.fy)), (cl(t.y0), cl(t.x0 + 1), t.fx * (1 - t.fy)),
                  (cl(t.y0 + 1), cl(t.x0), (1 - t.fx) * t.fy), (cl(t.y0 + 1), cl(t.x0 + 1), t.fx * t.fy)]
        # the taps a result depends on: those of the contributing pairs (no other pair has a weight in any image or gradient)
        t.tap_idx = [_tap_index(texture, t.face, yy, xx, t.contrib) for yy, xx, _ in t.taps]
        t.tex = sum(wt[..., None] * _texels(texture)[ix] for ix, (_, _, wt) in zip(t.tap_idx, t.taps))
        t.colarg = SH_C0 * t.tex + r[None, :, 17:20] + 0.5
    else:
        t.colarg = (r[None, :, 17:20] + 0.5).expand(P, K, 3) + torch.zeros(P, K, 3, dtype=dtype)
    t.fdepth = r[None, :, 20].expand(P, K) + torch.zeros(P, K, dtype=dtype)
    t.fnorm = r[None, :, 21:24].expand(P, K, 3) + torch.zeros(P, K, 3, dtype=dtype)
    col = t.colarg.clamp(min=0.0)
    t.color = (t.w[..., None] * col).sum(1) + t.Tfin[:, None] * case.bg.to(dtype)[None]
    t.color_abs = (t.w[..., None] * col).sum(1).detach() + t.Tfin.detach()[:, None] * case.bg.to(dtype)[None]
    t.depth = (t.w * t.fdepth).sum(1)
    t.depth_abs = (t.w * t.fdepth.abs()).sum(1).detach()
    t.norm = (t.w[..., None] * t.fnorm).sum(1)
    t.norm_abs = (t.w[..., None] * t.fnorm.abs()).sum(1).detach()
    t.alpha_img = t.w.sum(1)
    return t


# What an fp32 blend does to a pair beyond the fp32 statement's own figure, counted in roundings (2^-24) -- derived from the kernels'
# arithmetic, never fitted.  test_blend_gpu.py adds it only to the (case, output) pairs it names, in units of the output's sum|terms|,
# and never lets a bar grow past 1e-3 of that unit because of it:
#  * a contributor has alpha >= 1/255 and opacity <= 1, so power >= -ln 255 = -5.55; the three roundings of power and the scaling of
#    the argument inside __expf are each relative to |power|: 4 * 5.55 = 22 roundings of alpha, + 8 for the rest of the pair:
#    PAIR_ROUNDINGS = 30.
#  * the transmittance of a pair is a product of (1 - alpha_k) over the pixel's contributors: K6 forms final_T front to back (the
#    rounding of 1 - alpha and the product: 2 per contributor), K7 walks back from it as T <- T * rcp(1 - alpha) (the rounding of
#    1 - alpha, v_rcp_f32 = 1 ulp = 2 roundings, the product: 4), W_STEPS = 6 in all; and alpha's own PAIR_ROUNDINGS reach 1 - alpha
#    scaled by alpha.  Every one of them is a rounding of a number near 1 taken relative to 1 - alpha_k -- at the 0.99 clamp a
#    hundred times larger.  The DEPTH of a pixel is therefore sum over its contributors k of (W_STEPS + PAIR_ROUNDINGS alpha_k) /
#    (1 - alpha_k) roundings, carried by every w-linear term of every pair of that pixel.
#  * dL/dpower = alpha_raw (T s - (sum over the contributors behind of s_k w_k + T_final bg.dL/dcolour) / (1 - alpha)) is itself an
#    fp32 sum taken one contributor after the other: one rounding more per contributor of the pixel (P_STEPS = 1).  Where that sum
#    cancels, its error is relative to its elementary terms, not to |dL/dpower|; the bound is nevertheless stated relative to
#    |dL/dpower|, the unit of the M_P slots, and is then no upper bound but an estimate -- a row that misses it is a finding.
PAIR_ROUNDINGS, W_STEPS, P_STEPS = 30.0, 6.0, 1.0


def blend(case, dtype=F64, want_grads=True, colour_only=False, bg=None):
    """-> namespace: images color [3,H,W] depth [1,H,W] norm [3,H,W] alpha [1,H,W], final_T [H,W], n_contrib [H,W] (int64), *_abs the
    sums of |terms| of each image, pairs [H,W] the contributors per pixel, block_contrib [T,4] the Gaussians that contribute to each
    8x8 block; with want_grads: M / M_abs [N,32], M_n [N] (contributing pairs of the Gaussian), d_rec [N,24] (autograd on the record
    leaf), M_ext [N,32] (the constants above: sum|terms| weighted with the roundings each term carries), d_tex / d_tex_abs / d_tex_ext [6,R,R,3], d_tex_n [6,R,R] and d_tex_x [6,R,R,3], the sum of |dL/d(texture sample)| of the footprints
    that touch the texel whatever their tap weight (None without a texture; window-shaped, see Windows, where the texture is one).
    colour_only: only dL/dcolour is non-zero."""
    H, W, N = case.H, case.W, case.N
    if bg is not None:
        case = _with(case, bg=bg)
    rec = case.rec.to(dtype).clone().requires_grad_(want_grads)
    texture = None if case.texture is None else case.texture.to(dtype).clone().requires_grad_(want_grads)
    o = SimpleNamespace(color=torch.zeros(3, H, W, dtype=dtype), depth=torch.zeros(1, H, W, dtype=dtype), norm=torch.zeros(3, H, W, dtype=dtype),
                        alpha=torch.zeros(1, H, W, dtype=dtype), final_T=torch.ones(H, W, dtype=dtype), n_contrib=torch.zeros(H, W, dtype=torch.int64),
                        color_abs=torch.zeros(3, H, W, dtype=dtype), depth_abs=torch.zeros(1, H, W, dtype=dtype),
                        norm_abs=torch.zeros(3, H, W, dtype=dtype), pairs=torch.zeros(H, W, dtype=torch.int64),
                        block_contrib=torch.zeros(case.gx * case.gy, 4, dtype=torch.int64))
    if want_grads:
        o.M, o.M_abs, o.M_n = torch.zeros(N, ACC, dtype=dtype), torch.zeros(N, ACC, dtype=dtype), torch.zeros(N, dtype=torch.int64)
        o.M_ext = torch.zeros(N, ACC, dtype=dtype)
        if texture is not None:
            tv = _texels(texture)
            o.d_tex_abs, o.d_tex_n = torch.zeros_like(tv), torch.zeros(tv.shape[:-1], dtype=torch.int64)
            o.d_tex_x, o.d_tex_ext = torch.zeros_like(tv), torch.zeros_like(tv)
    up = {k: (v.to(dtype) if (k == "color" or not colour_only) else torch.zeros_like(v, dtype=dtype)) for k, v in case.up.items()}
    for tile in range(case.gx * case.gy):
        t = _tile_forward(case, tile, rec, texture, dtype)
        m, py, px = t.inside, t.py[t.inside], t.px[t.inside]
        with torch.no_grad():
            o.color[:, py, px], o.depth[0, py, px], o.norm[:, py, px] = t.color[m].t(), t.depth[m], t.norm[m].t()
            o.alpha[0, py, px], o.final_T[py, px], o.n_contrib[py, px] = t.alpha_img[m], t.Tfin[m], t.n_contrib[m]
            o.color_abs[:, py, px], o.depth_abs[0, py, px], o.norm_abs[:, py, px] = t.color_abs[m].t(), t.depth_abs[m], t.norm_abs[m].t()
            o.pairs[py, px] = t.contrib.sum(1)[m]
            for b in range(4):
                o.block_contrib[tile, b] = int(t.contrib[t.block == b].any(0).sum()) if t.K else 0
        if not want_grads or t.K == 0:
            continue
        keep = [t.power, t.fdepth, t.fnorm, t.colarg] + ([t.den, t.num, t.uv, t.tex] if texture is not None else [])
        for v in keep:
            v.retain_grad()
        loss = ((up["color"][:, py, px] * t.color[m].t()).sum() + (up["depth"][0, py, px] * t.depth[m]).sum()
                + (up["norm"][:, py, px] * t.norm[m].t()).sum() + (up["alpha"][0, py, px] * t.alpha_img[m]).sum())
        loss.backward()
        with torch.no_grad():
            terms = torch.zeros(t.px.numel(), t.K, ACC, dtype=dtype)
            Pg = t.power.grad
            for k, mono in enumerate([torch.ones_like(t.dx), t.dx, t.dy, t.dx * t.dx, t.dx * t.dy, t.dy * t.dy]):
                terms[..., PR.M_P + k] = Pg * mono
            if texture is not None:
                for k, mono in enumerate([torch.ones_like(t.dx), t.dpx, t.dpy]):
                    terms[..., PR.M_DEN + k] = t.den.grad * mono
                    for c in range(3):
                        terms[..., PR.M_DN + 3 * c + k] = t.num.grad[..., c] * mono
                terms[..., PR.M_PHI:PR.M_PHI + 3] = t.uv.grad
            terms[..., PR.M_VD:PR.M_VD + 3] = t.colarg.grad
            terms[..., PR.M_DEPTH] = t.fdepth.grad
            terms[..., PR.M_N:PR.M_N + 3] = t.fnorm.grad
            o.M.index_add_(0, t.ids, terms.sum(0))
            o.M_abs.index_add_(0, t.ids, terms.abs().sum(0))
            # M_ext (the comment above blend()): every term weighted with the depth of its pixel, in roundings
            nu = t.contrib.sum(1, keepdim=True).to(dtype)
            depth = torch.where(t.contrib, (W_STEPS + PAIR_ROUNDINGS * t.alpha) / (1.0 - t.alpha), torch.zeros_like(t.alpha)).sum(1, keepdim=True)
            ext = terms.abs() * (depth + PAIR_ROUNDINGS)[..., None]
            ext[..., PR.M_P:PR.M_P + 6] += terms[..., PR.M_P:PR.M_P + 6].abs() * (P_STEPS * nu)[..., None]
            o.M_ext.index_add_(0, t.ids, ext.sum(0))
            o.M_n.index_add_(0, t.ids, t.contrib.sum(0))
            if texture is not None:
                cm = t.contrib
                for ix, (yy, xx, wt) in zip(t.tap_idx, t.taps):
                    ix = tuple(i[cm] for i in ix)
                    o.d_tex_abs.index_put_(ix, (wt[cm][:, None] * t.tex.grad[cm]).abs(), accumulate=True)
                    o.d_tex_n.index_put_(ix, torch.ones(int(cm.sum()), dtype=torch.int64), accumulate=True)
                    o.d_tex_x.index_put_(ix, t.tex.grad[cm].abs(), accumulate=True)
                    o.d_tex_ext.index_put_(ix,
                                           (wt[cm][:, None] * t.tex.grad[cm]).abs() * (depth.expand_as(wt)[cm] + PAIR_ROUNDINGS)[:, None], accumulate=True)
    if want_grads:
        o.d_rec = rec.grad.detach() if rec.grad is not None else torch.zeros(N, REC, dtype=dtype)
        o.d_tex = None if texture is None else (_texels(texture).grad.detach() if _texels(texture).grad is not None else torch.zeros_like(_texels(texture)))
        if texture is None:
            o.d_tex_abs = o.d_tex_n = o.d_tex_x = o.d_tex_ext = None
    return o


def _with(case, **kw):
    c = Case.__new__(Case)
    c.__dict__.update(case.__dict__)
    c.__dict__.update(kw)
    return c


# ------------------------------------------------------------------------------------------------------- device records
def _round_up_f32(v64):
    f = v64.to(F32)
    low = f.to(F64) < v64
    return torch.where(low, torch.nextafter(f, torch.full_like(f, float("inf"))), f)


def cull_aids(rec):
    """thr = -ln(255 op) - 1e-3 (1 where op = 0: nothing can pass), rcull = 1.001 sqrt(-2 thr lam) + 0.01 (-1 where thr >= 0), lam the
    larger eigenvalue of cov2D = conic^-1 with K1's floor of 0.1 under the root; float64, rounded up to fp32"""
    r = rec.to(F64)
    ca, cb, cc, op = r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    det = 1.0 / (ca * cc - cb * cb)
    mid = 0.5 * (cc * det + ca * det)
    lam = mid + torch.sqrt((mid * mid - det).clamp_min(0.1))
    thr = torch.where(op > 0, -torch.log(255.0 * torch.where(op > 0, op, torch.ones_like(op))) - 1e-3, torch.ones_like(op))
    rcull = torch.where(thr < 0, torch.sqrt((-2.0 * thr * lam).clamp_min(0.0)) * 1.001 + 0.01, -torch.ones_like(op))
    return _round_up_f32(thr), _round_up_f32(rcull)


def device_records(case):
    """rec_test [N,8]: xy, conic pre-scaled by (-1/2, -1, -1/2) (exact in fp32), opacity, rcull, thr; rec_shade [N,20]: g, G, phi,
    viewdep, depth, normal, xy again"""
    r = case.rec
    thr, rcull = cull_aids(r) if getattr(case, "cull", None) is None else case.cull      # (case.cull: the values K1 itself wrote)
    test = torch.cat([r[:, 0:2], -0.5 * r[:, 2:3], -r[:, 3:4], -0.5 * r[:, 4:5], r[:, 5:6], rcull[:, None], thr[:, None]], 1)
    shade = torch.cat([r[:, 6:24], r[:, 0:2]], 1)
    return test.contiguous(), shade.contiguous()


# ------------------------------------------------------------------------------------------------------- decisions
def decision_gaps(case):
    """-> ({decision: smallest gap over the reached pairs}, offenders: bool [N] Gaussians with a pair below its bar, counters).
    alpha vs 1/255 (relative; at least 16 * 2^-24 * sum|terms of power| as well: the rounding of an fp32 power of that conditioning),
    T (1 - alpha) vs 1e-4, den vs DEN_MIN, the face choice, the colour argument vs 0 (relative to the sum of its |terms|), and the
    texel coordinate vs a bilinear cell edge in texels (bar R * 2^-20)."""
    rec = case.rec.to(F64)
    texture = None if case.texture is None else case.texture.to(F64)
    inf = float("inf")
    worst = {k: inf for k in ("alpha", "t_stop", "den", "face", "colour", "cell")}
    off = torch.zeros(case.N, dtype=torch.bool)
    cnt = dict(reached=0, contrib=0, alpha_raw_clamped=0, den_small=0, den_regular=0, channel_clamped=0, clamp_left=0, clamp_right=0,
               clamp_top=0, clamp_bottom=0, faces=set(), stopping=0, centre_outside_block=0, max_pairs_block=0, max_contrib_pixel=0)
    cnt["stop_blocks"] = set()
    cnt["bad_pairs"] = 0
    case.bad_pixels = torch.zeros(case.H, case.W, dtype=torch.bool)         # pixels that own a pair below its bar
    with torch.no_grad():
        for tile in range(case.gx * case.gy):
            t = _tile_forward(case, tile, rec, texture, F64)
            if t.K == 0:
                continue
            bad = torch.zeros_like(t.reached)
            g_alpha = (t.alpha - ALPHA_MIN).abs() / ALPHA_MIN
            need = torch.maximum(torch.full_like(g_alpha, GAP), 16.0 * EPS32 * t.power_scale / 1.0)
            sel = t.reached
            bad |= sel & (g_alpha < need)
            worst["alpha"] = min(worst["alpha"], float((g_alpha / (need / GAP))[sel].min()) if bool(sel.any()) else inf)
            g_t = (t.Tafter - T_EPS).abs() / T_EPS
            sel = t.ok
            bad |= sel & (g_t < GAP)
            worst["t_stop"] = min(worst["t_stop"], float(g_t[sel].min()) if bool(sel.any()) else inf)
            c = t.contrib
            if texture is not None:
                g_den = (t.den - DEN_MIN).abs() / DEN_MIN
                bad |= c & (g_den < GAP)
                bad |= c & (t.face_margin < GAP)
                edge = torch.minimum(torch.minimum(t.fx, 1 - t.fx), torch.minimum(t.fy, 1 - t.fy))
                bad |= c & (edge < case.R * 2.0 ** -20)
                if bool(c.any()):
                    worst["den"], worst["face"] = min(worst["den"], float(g_den[c].min())), min(worst["face"], float(t.face_margin[c].min()))
                    worst["cell"] = min(worst["cell"], float(edge[c].min()) / (case.R * 2.0 ** -20) * GAP)
                cnt["den_small"] += int((c & ~t.good).sum())
                cnt["den_regular"] += int((c & (t.den >= 0.25) & (t.den <= 4.0)).sum())
                R = case.R
                cnt["clamp_left"] += int((c & (t.x0 < 0)).sum())
                cnt["clamp_right"] += int((c & (t.x0 >= R - 1)).sum())
                cnt["clamp_top"] += int((c & (t.y0 < 0)).sum())
                cnt["clamp_bottom"] += int((c & (t.y0 >= R - 1)).sum())
                cnt["faces"] |= set(t.face[c].unique().tolist())
                scale = (SH_C0 * t.tex).abs() + rec[t.ids][None, :, 17:20].abs() + 0.5
            else:
                scale = rec[t.ids][None, :, 17:20].abs().expand_as(t.colarg) + 0.5
            g_col = (t.colarg.abs() / scale).min(-1).values
            bad |= c & (g_col < GAP)
            if bool(c.any()):
                worst["colour"] = min(worst["colour"], float(g_col[c].min()))
            off[t.ids[bad.any(0)]] = True
            cnt["bad_pairs"] += int(bad.sum())
            bp = bad.any(1) & t.inside
            case.bad_pixels[t.py[bp], t.px[bp]] = True
            cnt["reached"] += int(t.reached.sum())
            cnt["contrib"] += int(c.sum())
            cnt["alpha_raw_clamped"] += int((c & (t.araw > ALPHA_MAX)).sum())
            cnt["channel_clamped"] += int((c & (t.colarg < 0).any(-1)).sum())
            stop = t.ok & ~c
            cnt["stopping"] += int(stop.sum())
            for b in range(4):
                if bool(stop[t.block == b].any()):
                    cnt["stop_blocks"].add((tile, b))
                cnt["max_pairs_block"] = max(cnt["max_pairs_block"], int(c[t.block == b].sum()))
            cnt["max_contrib_pixel"] = max(cnt["max_contrib_pixel"], int(c.sum(1).max()))
            # the Gaussian's centre outside the pair's 8x8 block and outside its 4x4 quadrant
            bx0 = (t.px // 8 * 8).to(F64)[:, None]
            by0 = (t.py // 8 * 8).to(F64)[:, None]
            gx_, gy_ = rec[t.ids][None, :, 0], rec[t.ids][None, :, 1]
            outside = (gx_ < bx0) | (gx_ > bx0 + 7) | (gy_ < by0) | (gy_ > by0 + 7)
            cnt["centre_outside_block"] += int((c & outside).sum())
    cnt["faces"], cnt["stop_blocks"] = len(cnt["faces"]), len(cnt["stop_blocks"])
    return worst, off, cnt


def settle(case, seed, tries=40, phi_nudge=3e-3):
    """Nudge the Gaussians that own a pair within its bar of a threshold (opacity down by a few 2^-10, phi / viewdep / g by a few
    1e-3; phi_nudge: the large-R cases move phi by a hundredth of a texel instead, 3e-3 is five texels at R = 7168) until none is
    left; the values stay float32.  Asserts that every gap holds: nothing is excused at comparison time."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(tries):
        worst, off, cnt = decision_gaps(case)
        if not bool(off.any()):
            break
        n = int(off.sum())
        r = case.rec
        r[off, 5] = (r[off, 5] * (1.0 - 2.0 ** -10 * (1.0 + 3.0 * torch.rand(n, generator=g)))).to(F32)
        if case.texture is not None:
            r[off, 14:17] += phi_nudge * (torch.rand(n, 3, generator=g) - 0.5)
            r[off, 6:8] *= 1.0 + 4e-3 * (torch.rand(n, 2, generator=g) - 0.5)
        r[off, 17:20] += 4e-3 * (torch.rand(n, 3, generator=g) - 0.5)
    assert not bool(off.any()), (case.name, "gaps", worst, int(off.sum()))
    assert all(v >= GAP for v in worst.values()), (case.name, worst)
    case.gaps = worst
    case.counters.update({k: v for k, v in cnt.items()})
    return case


# ------------------------------------------------------------------------------------------------------- builders
def _rec(n):
    r = torch.zeros(n, REC, dtype=F32)
    r[:, 16] = 1.0                                   # phi = (0, 0, 1)
    return r


def _fill_common(g, r, textured, vd=0.3):
    n = r.shape[0]
    u = lambda *s: torch.rand(*s, generator=g)
    r[:, 17:20] = vd * (2 * u(n, 3) - 1)
    r[:, 20] = 0.5 + 4.0 * u(n)
    nv = torch.randn(n, 3, generator=g)
    r[:, 21:24] = nv / nv.norm(dim=1, keepdim=True)
    if textured:
        r[:, 6:8] = 0.02 * (2 * u(n, 2) - 1)
    return r


def direction(face, col, row, R):
    """the direction whose cubemap address is (face, col, row) in texels (the inverse of cube_address, major axis = 1)"""
    sc, tc = 2.0 * (col + 0.5) / R - 1.0, 2.0 * (row + 0.5) / R - 1.0
    sm = torch.where(face % 2 == 0, 1.0, -1.0)
    ax = face // 2
    x = torch.where(ax == 0, sm, torch.where(ax == 1, sc, sm * sc))
    y = torch.where(ax == 0, -tc, torch.where(ax == 1, sm, -tc))
    z = torch.where(ax == 0, -sm * sc, torch.where(ax == 1, sm * tc, sm))
    return torch.stack([x, y, z], -1)


def _uv_plane(g, r, R, face, col, row, texels_per_px):
    """phi at (face, col, row); G: a random 3x2 matrix that moves the address by about `texels_per_px` texels per pixel"""
    n = r.shape[0]
    r[:, 14:17] = direction(face, col, row, R).to(F32)
    r[:, 8:14] = (torch.randn(n, 6, generator=g) * (texels_per_px * 2.0 / R)[:, None]).to(F32)


def make_texture(g, R):
    return (1.5 * (2 * torch.rand(6, R, R, 3, generator=g) - 1)).to(F32)


def _single_tile(name, rec, texture, seed, W=16, H=16):
    n = rec.shape[0]
    return Case(name, W, H, rec, torch.arange(n), torch.tensor([[0, n]]), texture, seed)


def _wide(g, n, lo=0.02, hi=0.04, span=16.0):
    """wide splats of small alpha: sigma 20 px, every pixel of a 16x16 tile gets alpha >= 0.3 lo > 1/255, nobody saturates"""
    r = _rec(n)
    u = lambda *s: torch.rand(*s, generator=g)
    r[:, 0:2] = span * u(n, 2) - 0.5
    s2 = (18.0 + 6.0 * u(n)) ** 2
    r[:, 2], r[:, 4] = 1.0 / s2, 1.0 / (s2 * (0.8 + 0.4 * u(n)))
    r[:, 3] = 0.3 * (2 * u(n) - 1) * torch.sqrt(r[:, 2] * r[:, 4])
    r[:, 5] = lo + (hi - lo) * u(n)
    return r


def _small(g, n, block, op=(0.2, 0.6)):
    """small splats (sigma 0.5 px) whose rcull disc stays inside 8x8 block `block` [n] of the tile"""
    r = _rec(n)
    u = lambda *s: torch.rand(*s, generator=g)
    r[:, 0] = 8.0 * (block % 2) + 2.6 + 1.8 * u(n)
    r[:, 1] = 8.0 * (block // 2) + 2.6 + 1.8 * u(n)
    r[:, 2] = r[:, 4] = 4.0
    r[:, 5] = op[0] + (op[1] - op[0]) * u(n)
    return r


def disc_survivors(case):
    """[T,4] list entries whose rcull disc (float64, before the rounding up) touches the block's pixel rectangle: an upper bound of
    K6's survivors; for the entries of case a it is exact by construction (wide: contribute everywhere; small: inside one block)"""
    thr, rcull = cull_aids(case.rec)
    out = torch.zeros(case.gx * case.gy, 4, dtype=torch.int64)
    for tile in range(case.gx * case.gy):
        ids = case.point_list[int(case.ranges[tile, 0]):int(case.ranges[tile, 1])]
        x, y, rc = case.rec[ids, 0].to(F64), case.rec[ids, 1].to(F64), rcull[ids].to(F64)
        for b in range(4):
            x0, y0 = (tile % case.gx) * TILE + 8 * (b % 2), (tile // case.gx) * TILE + 8 * (b // 2)
            out[tile, b] = int(((rc >= 0) & (x + rc >= x0) & (x - rc <= x0 + 7) & (y + rc >= y0) & (y - rc <= y0 + 7)).sum())
    return out


LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]


def build_lengths(n, variant="all", textured=True):
    """case a: one tile, a list of exactly n entries.  `all`: every entry survives the cull of every block (n survivors per block:
    the ring wraps above 128, chunks of exactly 64 / 65 / 128 / 129).  `third`: every third entry is wide, the others are small
    splats inside one block each, so each block's survivor count differs from n and from its neighbours'."""
    seed = 1000 + 7 * n + (0 if variant == "all" else 3) + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    R = 64
    if variant == "all":
        r = _wide(g, n)
    else:
        k = torch.arange(n)
        r = _wide(g, n, lo=0.03, hi=0.05)
        sm = k % 3 != 0
        blk = torch.tensor([0, 1, 0, 2, 1, 0, 3, 2, 1, 0])[(k - k // 3) % 10]          # 4 : 3 : 2 : 1 over the blocks
        r[sm] = _small(g, int(sm.sum()), blk[sm])
    _fill_common(g, r, textured)
    if textured:
        face = torch.randint(0, 6, (n,), generator=g)
        _uv_plane(g, r, R, face, 4.0 + 56.0 * torch.rand(n, generator=g), 4.0 + 56.0 * torch.rand(n, generator=g), 0.15 + 0.2 * torch.rand(n, generator=g))
    case = _single_tile(f"len{n}_{variant}" + ("" if textured else "_untex"), r, make_texture(g, R) if textured else None, seed)
    settle(case, seed)
    ref = blend(case, want_grads=False)
    surv = disc_survivors(case)
    if variant == "all":
        assert bool((ref.block_contrib == n).all()) and bool((surv == n).all()), (n, ref.block_contrib)
        assert bool((ref.pairs == n).all())
    elif n >= 63:
        assert len(set(surv[0].tolist())) == 4 and int(surv.max()) < n, surv
        assert bool((ref.block_contrib[0] == surv[0]).all()), (ref.block_contrib, surv)
    if n >= 129 and variant == "all":
        assert case.counters["max_pairs_block"] > 128
    case.design["survivors"] = surv
    case.counters.update(list_length=n, survivors=surv[0].tolist())
    return case


def build_quadrants(textured=True):
    """case b: one tile.  60 small splats confined to quadrant 0 of block 0 (one quadrant list of 60, the others empty or short), 90
    more that each reach all 16 pixels of that quadrant and no other (segments beyond BWD_MAX_IT iterations and beyond 64 / 128 items), then an
    opaque layer that finishes three quadrants of block 0 early (tmax recomputation, rowdone) in front of a wide tail."""
    seed = 2000 + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    R = 64
    a = _rec(60)                                     # sigma 0.45 px inside pixels (0.8 .. 2.2) of quadrant 0: alpha < 1/255 beyond ~1.6 px
    a[:, 0:2] = 0.9 + 1.2 * u(60, 2)
    a[:, 2] = a[:, 4] = 5.0
    a[:, 5] = 0.05 + 0.1 * u(60)
    b = _rec(90)                                     # sigma 1 px at the quadrant's centre, small alpha: all 16 pixels of quadrant 0, none beyond
    b[:, 0:2] = 1.45 + 0.1 * u(90, 2)
    b[:, 2] = b[:, 4] = 1.0
    b[:, 5] = 0.05 + 0.02 * u(90)
    c = _rec(48)                                     # opaque, sigma 2 px, centred on quadrants 1..3 of block 0
    qc = torch.tensor([[5.5, 1.5], [1.5, 5.5], [5.5, 5.5]])[torch.arange(48) % 3]
    c[:, 0:2] = qc + 0.2 * (u(48, 2) - 0.5)
    c[:, 2] = c[:, 4] = 0.25
    c[:, 5] = 0.88 + 0.07 * u(48)
    d = _wide(g, 80, lo=0.016, hi=0.024)
    r = torch.cat([a, b, c, d], 0)
    n = r.shape[0]
    _fill_common(g, r, textured)
    if textured:
        _uv_plane(g, r, R, torch.randint(0, 6, (n,), generator=g), 4.0 + 56.0 * u(n), 4.0 + 56.0 * u(n), 0.1 + 0.2 * u(n))
    case = _single_tile("quadrants" + ("" if textured else "_untex"), r, make_texture(g, R) if textured else None, seed)
    settle(case, seed)
    # floors, from the float64 blend: Gaussians that reach quadrant 0 of block 0 / pairs there
    with torch.no_grad():
        t = _tile_forward(case, 0, case.rec.to(F64), None if case.texture is None else case.texture.to(F64), F64)
        q0 = (t.block == 0) & (t.quad == 0)
        per_quad = [int(t.contrib[(t.block == 0) & (t.quad == q)].any(0).sum()) for q in range(4)]
        pairs_q0 = int(t.contrib[q0].sum())
        done3 = [int(t.n_contrib[(t.block == 0) & (t.quad == q)].max()) for q in range(4)]
    assert per_quad[0] >= 40 + 17 and pairs_q0 >= 16 * 129, (per_quad, pairs_q0)
    assert max(done3[1:]) < n - 60 and done3[0] > max(done3[1:]), done3              # three quadrants finish early, quadrant 0 goes on
    case.counters.update(gaussians_per_quadrant=per_quad, pairs_quadrant0=pairs_q0, last_contributor_per_quadrant=done3)
    return case


def build_tstop(textured=True):
    """case c: stacks of three near-opaque splats on one pixel per block (stop after 3 entries), opaque splats of opacity 1 centred
    on pixels (alpha_raw > 0.99: the straight-through clamp), a broad opaque layer that finishes block 0, then a tail of 210 wide
    entries that the far block blends to the end."""
    seed = 3000 + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    R = 64
    a = _rec(12)
    for b in range(4):
        a[3 * b:3 * b + 3, 0] = 8.0 * (b % 2) + 6.0 + 0.05 * u(3)
        a[3 * b:3 * b + 3, 1] = 8.0 * (b // 2) + 6.0 + 0.05 * u(3)
        a[3 * b:3 * b + 3, 5] = torch.tensor([0.9, 0.98, 0.975])
    a[:, 2] = a[:, 4] = 2.0
    gx_, gy_ = torch.meshgrid(torch.arange(3), torch.arange(3), indexing="ij")
    cent = torch.stack([1.0 + 3.0 * gx_.reshape(-1), 1.0 + 3.0 * gy_.reshape(-1)], 1).to(F32)
    cent = torch.cat([cent, cent + torch.tensor([8.0, 0.0]), cent + torch.tensor([0.0, 8.0])], 0)
    b_ = _rec(27)
    b_[:, 0:2] = cent + 0.1 * (u(27, 2) - 0.5)
    b_[:, 2] = b_[:, 4] = 1.0 / 2.25
    b_[:, 5] = 1.0
    c = _rec(24)
    c[:, 0:2] = 3.5 + 1.0 * (u(24, 2) - 0.5)
    c[:, 2] = c[:, 4] = 1.0 / 16.0
    c[:, 5] = 0.9 + 0.08 * u(24)
    d = _wide(g, 210, lo=0.016, hi=0.024)
    r = torch.cat([a, b_, c, d], 0)
    n = r.shape[0]
    _fill_common(g, r, textured)
    if textured:
        _uv_plane(g, r, R, torch.randint(0, 6, (n,), generator=g), 4.0 + 56.0 * u(n), 4.0 + 56.0 * u(n), 0.1 + 0.2 * u(n))
    case = _single_tile("tstop" + ("" if textured else "_untex"), r, make_texture(g, R) if textured else None, seed)
    settle(case, seed)
    ref = blend(case, want_grads=False)
    nc = ref.n_contrib
    cn = case.counters
    assert cn["alpha_raw_clamped"] >= 20 and cn["stop_blocks"] == 4, cn
    assert int(nc[:8, :8].max()) <= n - 200, int(nc[:8, :8].max())                   # block 0 is all done while 200 entries remain
    assert int((nc == n).sum()) >= 16                                                  # others never stop
    with torch.no_grad():
        t = _tile_forward(case, 0, case.rec.to(F64), None if case.texture is None else case.texture.to(F64), F64)
        first_stop = torch.where((t.ok & ~t.contrib).any(1), (t.ok & ~t.contrib).to(torch.int64).argmax(1), torch.full((256,), n))
    assert int((first_stop <= 2).sum()) >= 1, "a pixel that stops at its third entry"
    cn.update(list_length=n, block0_last=int(nc[:8, :8].max()), never_stop_pixels=int((nc == n).sum()), stop_at_third=int((first_stop <= 2).sum()))
    return case


def build_needles(textured=True):
    """case d: edge-on splats (axis ratio 50 .. 80) at 10 .. 80 degrees whose centres lie outside an 8x8 block while the ridge clips a
    corner pixel of it; the set mirrored in x and in y.  One 16x16 tile: the four blocks' inner corners meet at (7.5, 7.5)."""
    seed = 4000 + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    R = 64
    base = []
    for k, deg in enumerate([10, 20, 30, 40, 50, 60, 70, 80] * 2):
        th = math.radians(deg)
        # the ridge passes through corner pixel (0, 0) of the tile (a corner of block 0 and of its quadrant 0); the centre sits on
        # the ridge 3 .. 9 px outside the tile, up-left of it
        dist = 3.0 + 6.0 * float(u(1))
        cx, cy = 0.0 - dist * math.cos(th) + 0.2 * float(u(1)), 0.0 - dist * math.sin(th) + 0.2 * float(u(1))
        s_long, ratio = 14.0 + 4.0 * float(u(1)), 50.0 + 30.0 * float(u(1))
        s_short = s_long / ratio
        c, s = math.cos(th), math.sin(th)
        il, is_ = 1.0 / s_long ** 2, 1.0 / s_short ** 2
        base.append([cx, cy, c * c * il + s * s * is_, c * s * (il - is_), s * s * il + c * c * is_, 0.5 + 0.45 * float(u(1))])
    base = torch.tensor(base, dtype=F64)
    rows = []
    for mx, my in ((0, 0), (1, 0), (0, 1), (1, 1)):
        m = base.clone()
        if mx:
            m[:, 0], m[:, 3] = 15.0 - m[:, 0], -m[:, 3]
        if my:
            m[:, 1], m[:, 3] = 15.0 - m[:, 1], -m[:, 3]
        rows.append(m)
    # the same needles pointing at the inner corners of the blocks: centre in the diagonally opposite block's far side
    inner = base.clone()
    inner[:, 0], inner[:, 1] = inner[:, 0] + 8.0, inner[:, 1] + 8.0                    # ridge through pixel (8, 8), centre up-left of it
    rows.append(inner)
    allr = torch.cat(rows, 0)
    n = allr.shape[0]
    r = _rec(n)
    r[:, 0:6] = allr.to(F32)
    _fill_common(g, r, textured)
    if textured:
        _uv_plane(g, r, R, torch.randint(0, 6, (n,), generator=g), 4.0 + 56.0 * u(n), 4.0 + 56.0 * u(n), 0.05 + 0.1 * u(n))
    case = _single_tile("needles" + ("" if textured else "_untex"), r, make_texture(g, R) if textured else None, seed)
    settle(case, seed)
    con = case.rec[:, 2:5].to(F64)
    ev = torch.linalg.eigvalsh(torch.stack([con[:, 0], con[:, 1], con[:, 1], con[:, 2]], 1).reshape(-1, 2, 2))
    assert float(torch.sqrt(ev[:, 1] / ev[:, 0]).min()) >= 50.0
    assert case.counters["centre_outside_block"] >= 30, case.counters
    case.counters.update(list_length=n, axis_ratio_min=float(torch.sqrt(ev[:, 1] / ev[:, 0]).min()))
    return case


def _disc_lists(case_W, case_H, rec):
    """every Gaussian is listed, in index order, in every tile its rcull disc touches"""
    gx, gy = (case_W + TILE - 1) // TILE, (case_H + TILE - 1) // TILE
    _, rcull = cull_aids(rec)
    x, y, rc = rec[:, 0].to(F64), rec[:, 1].to(F64), rcull.to(F64)
    pl, ranges = [], []
    for tile in range(gx * gy):
        x0, y0 = (tile % gx) * TILE, (tile // gx) * TILE
        hit = (rc >= 0) & (x + rc >= x0) & (x - rc <= x0 + 15) & (y + rc >= y0) & (y - rc <= y0 + 15)
        ids = torch.nonzero(hit).reshape(-1)
        ranges.append([sum(p.numel() for p in pl), sum(p.numel() for p in pl) + ids.numel()])
        pl.append(ids)
    return torch.cat(pl), torch.tensor(ranges, dtype=torch.int64)


SIZES = [(5, 3), (8, 8), (9, 17), (24, 40), (136, 88), (17, 129), (48, 33)]


def build_image(W, H, textured=True):
    """case e: an image that is no multiple of the tile, splats of 1.5 .. 5 px everywhere on the TILE GRID (so that blocks wholly
    outside the image have lists too), every tile's list non-empty"""
    seed = 5000 + 131 * W + H + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    R = 40
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    n = 14 * gx * gy + 10
    r = _rec(n)
    r[:, 0], r[:, 1] = 16.0 * gx * u(n) - 0.5, 16.0 * gy * u(n) - 0.5
    s1, s2 = 1.5 + 3.5 * u(n), 1.5 + 3.5 * u(n)
    th = math.pi * u(n)
    c, s = torch.cos(th), torch.sin(th)
    r[:, 2], r[:, 3], r[:, 4] = c * c / s1 ** 2 + s * s / s2 ** 2, c * s * (1 / s1 ** 2 - 1 / s2 ** 2), s * s / s1 ** 2 + c * c / s2 ** 2
    r[:, 5] = 0.1 + 0.8 * u(n)
    _fill_common(g, r, textured)
    if textured:
        _uv_plane(g, r, R, torch.randint(0, 6, (n,), generator=g), 3.0 + 34.0 * u(n), 3.0 + 34.0 * u(n), 0.1 + 0.3 * u(n))
    pl, ranges = _disc_lists(W, H, r)
    case = Case(f"image{W}x{H}" + ("" if textured else "_untex"), W, H, r, pl, ranges, make_texture(g, R) if textured else None, seed)
    settle(case, seed)
    lens = (case.ranges[:, 1] - case.ranges[:, 0])
    assert int(lens.min()) >= 1, "lists in every tile"
    case.counters.update(tiles=gx * gy, list_min=int(lens.min()), list_max=int(lens.max()),
                         blocks_outside=sum(1 for t in range(gx * gy) for b in range(4)
                                            if (t % gx) * 16 + 8 * (b % 2) >= W or (t // gx) * 16 + 8 * (b // 2) >= H))
    return case


RESOLUTIONS = [8, 33, 40, 96]


def build_uv(R):
    """case f: one tile, footprints on all six faces and within half a texel of all four borders of a face (clamped taps: the
    direct-scatter path), splats whose pairs straddle two faces, den below DEN_MIN and in [0.25, 4], a non-symmetric G, and negative
    viewdep so that colour channels clamp at 0."""
    seed = 6000 + R
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    n = 96
    r = _rec(n)
    r[:, 0:2] = 16.0 * u(n, 2) - 0.5
    s2 = (2.5 + 4.0 * u(n)) ** 2
    r[:, 2], r[:, 4] = 1.0 / s2, 1.0 / (s2 * (0.6 + 0.8 * u(n)))
    r[:, 3] = 0.5 * (2 * u(n) - 1) * torch.sqrt(r[:, 2] * r[:, 4])
    r[:, 5] = 0.05 + 0.3 * u(n)
    _fill_common(g, r, True, vd=0.3)
    k = torch.arange(n)
    face = k % 6
    col, row = 1.0 + (R - 3.0) * u(n), 1.0 + (R - 3.0) * u(n)
    speed = 0.1 + 0.3 * u(n)
    border = (k >= 24) & (k < 56)                       # 8 per border: address within half a texel of it, nearly at rest
    side = (k - 24) % 4
    col = torch.where(border & (side == 0), -0.25 - 0.1 * u(n), torch.where(border & (side == 1), R - 0.75 + 0.1 * u(n), col))
    row = torch.where(border & (side == 2), -0.25 - 0.1 * u(n), torch.where(border & (side == 3), R - 0.75 + 0.1 * u(n), row))
    speed = torch.where(border, 0.004 * torch.ones(n), speed)
    straddle = (k >= 56) & (k < 72)                     # one texel inside an edge, moving: pairs on both faces
    col = torch.where(straddle, torch.where(k % 2 == 0, 1.0 + 0.5 * u(n), R - 2.5 + 0.5 * u(n)), col)
    speed = torch.where(straddle, 0.5 * torch.ones(n), speed)
    _uv_plane(g, r, R, face, col, row, speed)
    steep = (k >= 72) & (k < 84)                        # den = 1 + g.dp sweeps through DEN_MIN inside the tile
    r[steep, 6:8] = (0.12 * (2 * u(int(steep.sum()), 2) - 1)).to(F32)
    r[k % 4 == 1, 17:20] -= 0.6                         # negative viewdep: clamped channels
    case = _single_tile(f"uv_R{R}", r, make_texture(g, R), seed)
    settle(case, seed)
    cn = case.counters
    assert cn["faces"] == 6, cn
    for b in ("clamp_left", "clamp_right", "clamp_top", "clamp_bottom"):
        assert cn[b] >= 10, (b, cn)
    assert cn["den_small"] >= 20 and cn["den_regular"] >= 20 and cn["channel_clamped"] >= 20, cn
    G = case.rec[:, 8:14].reshape(n, 3, 2)
    assert float((G[:, 0, 1] - G[:, 1, 0]).abs().min()) > 0, "G is not symmetric"
    return case


def build_uv_320():
    """one tile, 60 entries, R = 320 (10 bins per face row): footprints around columns 10 and 270 of one face -- bins x = 0 and
    x = 8 share the reservation table's home entry, a same-face collision"""
    seed = 6320
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    n, R = 60, 320
    r = _rec(n)
    r[:, 0:2] = 16.0 * u(n, 2) - 0.5
    s2 = (3.0 + 4.0 * u(n)) ** 2
    r[:, 2] = r[:, 4] = 1.0 / s2
    r[:, 5] = 0.05 + 0.2 * u(n)
    _fill_common(g, r, True)
    k = torch.arange(n)
    _uv_plane(g, r, R, torch.zeros(n, dtype=torch.int64), torch.where(k % 2 == 0, 6.0 + 16.0 * u(n), 262.0 + 16.0 * u(n)), 40.0 + 16.0 * u(n),
              0.2 + 0.2 * u(n))
    case = _single_tile("uv_R320", r, make_texture(g, R), seed)
    settle(case, seed)
    with torch.no_grad():
        t = _tile_forward(case, 0, case.rec.to(F64), case.texture.to(F64), F64)
        bx = (t.x0.clamp(0, R - 1) // 32)[t.contrib]
    assert int((bx == 0).sum()) >= 100 and int((bx == 8).sum()) >= 100
    case.counters.update(pairs_bin_x0=int((bx == 0).sum()), pairs_bin_x8=int((bx == 8).sum()))
    return case


BIG_RESOLUTIONS = [2368, 5462, 7168]
BIG_WINDOW = 96
BIG_ORIGINS = {1: (301, 1207), 2: (1739, 85), 3: (911, 2011), 4: (2125, 1499)}     # (y0, x0) of faces 1..4 at every R: no multiple of 32
# Inside the windows make_texture's +-1.5 white noise is divided by 64 and rides on +-1.5 noise of 8-texel cells, bilinearly
# interpolated.  The float32 statement's address is off by about R 2^-23 texel (5e-4 at R = 7168), the same for all pairs of an
# address at rest: `color` moves by that times the step between neighbouring texels, and the UV-chain moments (dL/dcol is a
# difference of texels weighted with the other axis' fraction) by that times |second difference| / |first difference| of the cell,
# which has no bound in white noise (measured: 1.2e-3 of sum|terms| at R = 7168 with white noise / 8, over the 1e-3 cap).
BIG_CONTRAST = 1.0 / 64.0


def big_window_block(g, size=BIG_WINDOW):
    coarse = 1.5 * (2 * torch.rand(1, 3, size // 8 + 1, size // 8 + 1, generator=g, dtype=F64) - 1)
    smooth = torch.nn.functional.interpolate(coarse, size=(size + 1, size + 1), mode="bilinear", align_corners=True)[0, :, :size, :size]
    return (smooth.permute(1, 2, 0) + BIG_CONTRAST * 1.5 * (2 * torch.rand(size, size, 3, generator=g, dtype=F64) - 1)).to(F32)
BIN_CHUNK = 32768                 # bins per trip of k_bin_offsets' loop (1024 threads x BO_MAX)


def big_origins(R):
    return [(0, 0)] + [BIG_ORIGINS[f] for f in (1, 2, 3, 4)] + [(R - BIG_WINDOW, R - BIG_WINDOW)]


def build_uv_big(R):
    """one tile, 96 entries, 16 per face, a 96x96-texel window per face of a texture of nominal resolution R (2368: the second trip
    of k_bin_offsets' loop; 5462: the first allocation past 2^31 bytes; 7168: the limit of the ABI).  Face 0's window is the
    top-left corner with footprints clamped at the left and top borders (one in the corner: texel 0), face 5's the bottom-right
    corner with footprints clamped at the right and bottom borders (one in the corner: the last texel of the allocation) and
    footprints in its last 8 rows and above them; the others lie inside their faces.  Nearly every address is at rest (a few 1e-3
    texel per pixel, the fraction well inside its cell), four small fast splats per inner face sweep several cells: the cell bar
    R 2^-20 texel is 6.8e-3 at R = 7168, and a large splat whose address sweeps many texels never settles."""
    seed = 6000 + R
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    n = 96
    r = _rec(n)
    r[:, 0:2] = 16.0 * u(n, 2) - 0.5
    s2 = (2.5 + 4.0 * u(n)) ** 2
    r[:, 2], r[:, 4] = 1.0 / s2, 1.0 / (s2 * (0.6 + 0.8 * u(n)))
    r[:, 3] = 0.5 * (2 * u(n) - 1) * torch.sqrt(r[:, 2] * r[:, 4])
    r[:, 5] = 0.05 + 0.3 * u(n)
    k = torch.arange(n)
    face, j = k % 6, k // 6
    fast = (face >= 1) & (face <= 4) & (j >= 12)          # sigma 0.5 px: a dozen pairs each, 0.3 texel per pixel
    r[fast, 2] = r[fast, 4] = 4.0
    r[fast, 3] = 0.0
    r[fast, 5] = (0.3 + 0.4 * u(n))[fast]
    r[fast, 0:2] = (2.0 + 12.0 * u(n, 2))[fast]
    _fill_common(g, r, True, vd=0.3)
    org = torch.tensor(big_origins(R), dtype=F64)
    frac = lambda: 0.25 + 0.5 * u(n).to(F64)
    lrow = torch.floor(12.0 + 72.0 * u(n)).to(F64) + frac()                      # inside the window, in texels from its origin
    lcol = torch.floor(12.0 + 72.0 * u(n)).to(F64) + frac()
    f5 = face == 5
    lrow = torch.where(f5 & (j >= 12) & (j < 14), torch.floor(88.0 + 6.0 * u(n)).to(F64) + frac(), lrow)     # the last 8 rows, not clamped
    lrow = torch.where(f5 & (j == 14), torch.floor(6.0 + 20.0 * u(n)).to(F64) + frac(), lrow)                # the window's first bin row
    lrow = torch.where(f5 & (j == 15), torch.floor(40.0 + 20.0 * u(n)).to(F64) + frac(), lrow)
    f0 = face == 0
    lrow = torch.where(f0 & (j >= 12) & (j < 14), torch.floor(4.0 + 24.0 * u(n)).to(F64) + frac(), lrow)     # bin 0
    lcol = torch.where(f0 & (j >= 12) & (j < 14), torch.floor(4.0 + 24.0 * u(n)).to(F64) + frac(), lcol)
    row, col = org[face, 0] + lrow, org[face, 1] + lcol
    # within half a texel of a border (both taps on one texel), yet GAP clear of the face edge: half a texel is 1.4e-4 of the major
    # axis at R = 7168, so the address sits 0.41 .. 0.47 texel from the edge there (0.2 .. 0.47 at R = 2368), at rest
    m_lo = max(0.2, 1.15 * GAP * 0.5 * R)
    m = lambda: m_lo + (0.47 - m_lo) * u(n).to(F64)
    lo, hi = -0.5 + m(), R - 0.5 - m()
    col = torch.where((face == 0) & (j < 6), lo, torch.where(f5 & (j < 6), hi, col))
    row = torch.where((face == 0) & ((j == 0) | ((j >= 6) & (j < 12))), lo, torch.where(f5 & ((j == 0) | ((j >= 6) & (j < 12))), hi, row))
    speed = torch.where(fast, 0.3 * torch.ones(n), 0.001 + 0.002 * u(n))
    speed = torch.where((f0 | f5) & (j < 12), 5e-5 + 5e-5 * u(n), speed)
    r[:, 14:17] = direction(face, col, row, R).to(F32)
    r[:, 8:14] = (torch.randn(n, 6, generator=g) * (speed * 2.0 / R)[:, None]).to(F32)
    r[k % 4 == 1, 17:20] -= 0.6                         # negative viewdep: clamped channels
    case = _single_tile(f"uv_big_R{R}", r, Windows(R, big_origins(R), [big_window_block(g) for _ in range(6)]), seed)
    settle(case, seed, phi_nudge=0.02 * 2.0 / R)
    cn = case.counters
    with torch.no_grad():
        t = _tile_forward(case, 0, case.rec.to(F64), case.texture.to(F64), F64)
        c = t.contrib
        on = lambda f, m: int((c & (t.face == f) & m).sum())
        cn.update(clamp_left_face0=on(0, t.x0 < 0), clamp_top_face0=on(0, t.y0 < 0), clamp_right_face5=on(5, t.x0 >= R - 1),
                  clamp_bottom_face5=on(5, t.y0 >= R - 1), first_texel=on(0, (t.x0 < 0) & (t.y0 < 0)),
                  last_texel=on(5, (t.x0 >= R - 1) & (t.y0 >= R - 1)))
        binned = c & (t.x0 >= 0) & (t.x0 < R - 1) & (t.y0 >= 0) & (t.y0 < R - 1)
        nb = (R + 31) // 32
        bins = ((t.face * nb + t.y0 // 32) * nb + t.x0 // 32)[binned]
        byte = (((t.face * R + t.y0) * R + t.x0) * 12)[binned]
        cn.update(bins=6 * nb * nb, pairs_binned=int(binned.sum()), pairs_bin0=int((bins == 0).sum()), pairs_below_chunk=int((bins < BIN_CHUNK).sum()),
                  pairs_above_chunk=int((bins >= BIN_CHUNK).sum()), pairs_below_2_31=int((byte < 2 ** 31).sum()),
                  pairs_above_2_31=int((byte >= 2 ** 31).sum()), pairs_face5_row_above_2_31=on(5, binned & (t.y0 * R * 12 + 5 * R * R * 12 >= 2 ** 31)),
                  last_byte_offset=(6 * R * R - 1) * 12)
    assert cn["faces"] == 6, cn
    for b in ("clamp_left_face0", "clamp_top_face0", "clamp_right_face5", "clamp_bottom_face5"):
        assert cn[b] >= 10, (b, cn)
    assert cn["first_texel"] >= 1 and cn["last_texel"] >= 1, cn
    assert cn["channel_clamped"] >= 20, cn
    assert 6 * nb * nb > BIN_CHUNK and cn["pairs_bin0"] >= 10 and cn["pairs_below_chunk"] >= 100 and cn["pairs_above_chunk"] >= 100, cn
    if 6 * R * R * 12 > 2 ** 31:
        assert cn["pairs_below_2_31"] >= 100 and cn["pairs_above_2_31"] >= 100, cn
    if R == 5462:                                       # byte 2^31 is texel (5, 5454, 2): footprints in the window's rows on both sides of it
        assert cn["pairs_face5_row_above_2_31"] >= 10 and on(5, binned & (t.y0 < 5453)) >= 10, cn
    return case


COUNT_LENGTHS = [1023, 1024, 1100]


def build_counts(n):
    """case g: W = H = 8 (one block), R = 64, every footprint in one texture bin; n entries of opacity 0.0045 .. 0.006 and conic
    a = c = 1e-4, each contributing to all 64 pixels: 64 n footprints in one (block, bin) reservation entry of 16 bits"""
    seed = 7000 + n
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    R = 64
    r = _rec(n)
    r[:, 0:2] = 1.5 + 4.0 * u(n, 2)
    r[:, 2] = r[:, 4] = 1e-4
    r[:, 5] = 0.0045 + 0.0015 * u(n)
    _fill_common(g, r, True)
    r[:, 6:8] = 0.0
    _uv_plane(g, r, R, 4 * torch.ones(n, dtype=torch.int64), 12.0 + 8.0 * u(n), 12.0 + 8.0 * u(n), 0.05 + 0.05 * u(n))
    case = _single_tile(f"counts{n}", r, make_texture(g, R), seed, W=8, H=8)
    settle(case, seed)
    ref = blend(case, want_grads=False)
    assert bool((ref.pairs == n).all()) and float(ref.final_T.min()) > 1e-3, float(ref.final_T.min())     # (exp(-6.6) = 1.4e-3: an order above T_EPS)
    with torch.no_grad():
        t = _tile_forward(case, 0, case.rec.to(F64), case.texture.to(F64), F64)
        c = t.contrib
        assert float((t.alpha[c] - ALPHA_MIN).min()) >= 1e-4
        assert bool(((t.x0[c] >= 0) & (t.x0[c] < 31) & (t.y0[c] >= 0) & (t.y0[c] < 31) & (t.face[c] == 4)).all()), "one bin"
    case.counters.update(footprints=64 * n, wrapped_count=(64 * n) & 0xFFFF, final_T_min=float(ref.final_T.min()))
    return case


CASES = {}
for _n in LENGTHS:
    CASES[f"len{_n}_all"] = functools.partial(build_lengths, _n, "all")
    if _n >= 63:
        CASES[f"len{_n}_third"] = functools.partial(build_lengths, _n, "third")
CASES["quadrants"] = build_quadrants
CASES["tstop"] = build_tstop
CASES["needles"] = build_needles
for _W, _H in SIZES:
    CASES[f"image{_W}x{_H}"] = functools.partial(build_image, _W, _H)
for _R in RESOLUTIONS:
    CASES[f"uv_R{_R}"] = functools.partial(build_uv, _R)
CASES["uv_R320"] = build_uv_320
for _R in BIG_RESOLUTIONS:
    CASES[f"uv_big_R{_R}"] = functools.partial(build_uv_big, _R)
for _n in COUNT_LENGTHS:
    CASES[f"counts{_n}"] = functools.partial(build_counts, _n)
for _n in (64, 65, 129):                                                      # case h: untextured
    CASES[f"len{_n}_all_untex"] = functools.partial(build_lengths, _n, "all", False)
CASES["tstop_untex"] = functools.partial(build_tstop, False)
for _W, _H in SIZES:
    CASES[f"image{_W}x{_H}_untex"] = functools.partial(build_image, _W, _H, False)
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """The case and its float64 blend (all four upstream gradients, the case's background) -- computed once per process, shared by
    every test, never modified."""
    case = CASES[name]()
    return SimpleNamespace(case=case, ref=blend(case))


@functools.lru_cache(maxsize=None)
def prepared_colour_only(name):
    """the null-pointer combination: dL/ddepth, dL/dnorm and dL/dalpha absent (zero), the case's non-zero background"""
    return blend(prepared(name).case, colour_only=True)


# ------------------------------------------------------------------------------------------------------- error measures and bars
def unit_error(got, ref, ref_abs):
    """worst |got - ref| in units of the output's sum of |terms| (a term-less output must be exactly its reference)"""
    g, e, a = torch.as_tensor(got).to(F64).reshape(-1), ref.to(F64).reshape(-1), ref_abs.to(F64).reshape(-1)
    if e.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    d = (g - e).abs()
    zero = a == 0
    if bool((d[zero] > 0).any()):
        return float("inf")
    return float((d[~zero] / a[~zero]).max()) if bool((~zero).any()) else 0.0


def over_bar(got, ref, ref_abs, n_terms, base):
    """worst (|got - ref| / sum|terms|) / (base + n 2^-24): <= 1 is within the bar of an fp32 sum of n terms taken in any order"""
    g, e, a = torch.as_tensor(got).to(F64).reshape(-1), ref.to(F64).reshape(-1), ref_abs.to(F64).reshape(-1)
    n = n_terms.to(F64).reshape(-1)
    if e.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    d = (g - e).abs()
    zero = a == 0
    if bool((d[zero] > 0).any()):
        return float("inf")
    return float((d[~zero] / a[~zero] / (base + n[~zero] * EPS32)).max()) if bool((~zero).any()) else 0.0


PARITY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "blend_parity.json")


def load_parity():
    try:
        with open(PARITY_JSON) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def store_parity(section, figures):
    """merge {case: {output: figure}} into `section` of profiles/blend_parity.json (three significant digits)"""
    if not figures:
        return
    doc = load_parity()
    sec = doc.setdefault(section, {})
    for name, by_output in figures.items():
        old = sec.setdefault(name, {})
        for k, v in by_output.items():
            # the float32 statement is deterministic on one machine (blend_f32), but the order of its parallel reductions follows the
            # thread count, and the device's float atomics take their terms in a varying order: a figure that moved by less than
            # 2 % is the same figure, and the file (whose "f32_statement" the bars are read from) stays
            if k not in old or abs(v - old[k]) > 0.02 * max(abs(old[k]), 1e-30):
                old[k] = float(f"{v:.3e}")
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    try:
        if not os.path.exists(PARITY_JSON) or open(PARITY_JSON).read() != text:
            with open(PARITY_JSON, "w") as f:
                f.write(text)
    except OSError:
        pass


def blend_f32(case):
    """blend() in float32 with torch's deterministic scatter-adds: the parallel ones take duplicate indices in a varying order, and
    the figures that the bars are made from would move from run to run"""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        return blend(case, dtype=F32)
    finally:
        torch.use_deterministic_algorithms(was)


@functools.lru_cache(maxsize=None)
def statement_figures(name):
    """blend() in float32 against itself in float64: per image and per moment slot the worst error in units of the slot's
    sum|terms| -- the basis of the bars"""
    p = prepared(name)
    case, ref = p.case, p.ref
    f = blend_f32(case)
    figs = {}
    for k in ("color", "depth", "norm"):
        figs[k] = unit_error(getattr(f, k), getattr(ref, k), getattr(ref, k + "_abs"))
    figs["alpha"] = unit_error(f.alpha, ref.alpha, ref.alpha)
    figs["final_T"] = unit_error(f.final_T, ref.final_T, ref.final_T)
    for s, nm in enumerate(MOMENT_NAMES):
        figs["M_" + nm] = unit_error(f.M[:, s], ref.M[:, s], ref.M_abs[:, s])
    if ref.d_tex is not None:
        figs["d_tex"] = unit_error(f.d_tex, ref.d_tex, ref.d_tex_abs)
        # a tap weight's own rounding error is absolute (R 2^-24 texels, whatever the weight), so a texel reached only through tiny
        # weights dominates the figure above; the second unit, the sum of |dL/d(sample)| of the footprints that touch the texel, is
        # the one a wrong footprint shows in.  The device is held to both.
        figs["d_tex_x"] = unit_error(f.d_tex, ref.d_tex, ref.d_tex_x)
    figs["n_contrib_equal"] = float(torch.equal(f.n_contrib, ref.n_contrib))
    return figs


@functools.lru_cache(maxsize=None)
def statement_figures_colour_only(name):
    """statement_figures() of the colour-only pass (dL/ddepth, dL/dnorm, dL/dalpha absent): the moment slots and the texture
    gradient.  There dL/dpower is made of colour terms alone, and a colour carries the float32 error of its tap address,
    R 2^-23 texel times the step between texels: at R >= 5462 the M_P slots of that pass stand at 4e-5 .. 8e-5 of sum|terms| in the
    float32 statement itself, 4 .. 8 x their figures in the full pass, where the depth / normal / alpha terms dilute them (with a
    constant texture they are 4e-7 .. 8e-7 in both)."""
    ref, f = prepared_colour_only(name), None
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        f = blend(prepared(name).case, dtype=F32, colour_only=True)
    finally:
        torch.use_deterministic_algorithms(was)
    figs = {"M_" + nm: unit_error(f.M[:, s], ref.M[:, s], ref.M_abs[:, s]) for s, nm in enumerate(MOMENT_NAMES)}
    if ref.d_tex is not None:
        figs["d_tex"], figs["d_tex_x"] = unit_error(f.d_tex, ref.d_tex, ref.d_tex_abs), unit_error(f.d_tex, ref.d_tex, ref.d_tex_x)
    figs["n_contrib_equal"] = float(torch.equal(f.n_contrib, ref.n_contrib))
    return figs


def base_bar(name, output, section="f32_statement"):
    """max(4 x the f32 statement's figure of that case and output, 8 * 2^-24): the factor 4 is the margin preprocess_ref.hip_bar uses
    (device exp / reciprocal / fused multiply-adds differ from the host's by a few ulp through the same chain)"""
    return max(4.0 * load_parity()[section][name][output], FLOOR)
