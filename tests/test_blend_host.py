"""K6 / K7 alone, on the CPU: the float64 statement of blend_ref.py agrees with oracle.texgs_torch.render + autograd to 1e-10 (images,
final_T, the record and texture gradients; n_contrib identical), its moment sums turn into autograd's dL/d(record) through
preprocess_ref.cotangent_from_moments to 1e-10 (the M_* definitions of csrc/common.h, pinned a second way), every builder holds its
floors and gaps, and the same statement evaluated in float32 -- the basis of the bars of test_blend_gpu.py -- takes every decision
as float64 does.  The float32 figures go to profiles/blend_parity.json under "f32_statement".
The windowed texture of the large-R cases (blend_ref.Windows) is held to the dense one bit for bit on a case that has both, and a
window misplaced by one texel must show in `color` and in dL/dtexture at 30 x their bars."""
import pytest
import torch

import blend_ref as B
import helpers as Hh
import preprocess_ref as PR
from oracle import texgs_torch as O

F64 = torch.float64
ALL = pytest.mark.parametrize("name", B.NAMES)
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    B.store_parity("f32_statement", _FIGURES)


@ALL
def test_builder_floors_and_gaps(name):
    """the builder's own assertions (its reached-edge floors, every decision of every reached pair >= GAP clear of its threshold);
    at most 3 x 3 tiles and about 1 200 entries per list; the counters are printed"""
    case = B.prepared(name).case
    print("BLEND CASE", name, case.counters, {k: float(f"{v:.3g}") for k, v in case.gaps.items()})
    assert all(v >= B.GAP for v in case.gaps.values()), case.gaps
    lens = case.ranges[:, 1] - case.ranges[:, 0]
    assert int(lens.max()) <= 1200 and (case.gx * case.gy <= 9 or name.startswith("image")), (int(lens.max()), case.gx, case.gy)
    assert bool((case.rec.to(F64).to(torch.float32) == case.rec).all()), "record values are fp32 numbers"


@ALL
def test_cull_aids_cover_every_contributor(name):
    """thr / rcull as uploaded: rounded up from float64, and the rcull disc of every Gaussian touches every 8x8 block it contributes
    to in float64 (else a missing contribution would be the record's fault, not the kernel's)"""
    case = B.prepared(name).case
    thr, rcull = B.cull_aids(case.rec)
    r = case.rec.to(F64)
    op = r[:, 5]
    thr64 = torch.where(op > 0, -torch.log(255.0 * op.clamp_min(1e-300)) - 1e-3, torch.ones_like(op))
    assert bool((thr.to(F64) >= thr64).all()) and bool(((thr.to(F64) - thr64).abs() <= 2.0 ** -23 * thr64.abs().clamp_min(1.0)).all())
    with torch.no_grad():
        for tile in range(case.gx * case.gy):
            t = B._tile_forward(case, tile, r, None if case.texture is None else case.texture.to(F64), F64)
            if t.K == 0:
                continue
            x, y, rc = r[t.ids, 0], r[t.ids, 1], rcull[t.ids].to(F64)
            for b in range(4):
                x0, y0 = (tile % case.gx) * 16 + 8 * (b % 2), (tile // case.gx) * 16 + 8 * (b // 2)
                disc = (rc >= 0) & (x + rc >= x0) & (x - rc <= x0 + 7) & (y + rc >= y0) & (y - rc <= y0 + 7)
                assert bool(disc[t.contrib[t.block == b].any(0)].all()), (tile, b)


def _oracle(case, colour_only=False):
    rec = case.rec.to(F64).clone().requires_grad_(True)
    textured = case.texture is not None
    tex = (case.texture.to(F64) if textured else torch.zeros(6, 4, 4, 3, dtype=F64)).clone().requires_grad_(True)
    pre = B.pre_from_rec(rec)
    pre["grid"] = (case.gx, case.gy)
    st = SimpleSettings(case)
    out, final_T, n_contrib, _ = O.render(pre, dict(point_list=case.point_list, ranges=case.ranges), tex, st, F64)
    up = case.up
    L = (up["color"].to(F64) * out[0:3]).sum()
    if not colour_only:
        L = L + (up["depth"].to(F64) * out[3:4]).sum() + (up["norm"].to(F64) * out[4:7]).sum() + (up["alpha"].to(F64) * out[7:8]).sum()
    L.backward()
    return out.detach(), final_T, n_contrib, rec.grad, (tex.grad if textured else None)


class SimpleSettings:
    def __init__(self, case):
        self.image_height, self.image_width, self.bg = case.H, case.W, case.bg


def _close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("name", ["len65_all", "tstop", "uv_R40", "len65_all_untex", "tstop_untex", "image9x17_untex", "needles", "quadrants"])
@pytest.mark.parametrize("colour_only", [False, True])
def test_statement_against_oracle(name, colour_only):
    p = B.prepared(name)
    case = p.case
    ref = B.prepared_colour_only(name) if colour_only else p.ref
    out, final_T, n_contrib, d_rec, d_tex = _oracle(case, colour_only)
    for k, (a, b) in {"color": (0, 3), "depth": (3, 4), "norm": (4, 7), "alpha": (7, 8)}.items():
        _close(getattr(ref, k), out[a:b], k)
    _close(ref.final_T, final_T, "final_T")
    assert torch.equal(ref.n_contrib, n_contrib)
    _close(ref.d_rec, d_rec, "d_rec")
    if d_tex is not None:
        _close(ref.d_tex, d_tex, "d_tex")
    else:
        assert not ref.M[:, B.UV_SLOTS].any() and not ref.d_rec[:, 6:17].any()
    # the moment definitions, a second way: M -> dL/d(record) by the map K8 is held to
    A = PR.cotangent_from_moments(ref.M, B.pre_from_rec(case.rec.to(F64)), textured=True)
    assert float(d_rec.abs().max()) > 0
    _close(A, d_rec, "cotangent_from_moments")
    assert not ref.M[~case.in_lists()].any() and not ref.M[:, 28:].any()


@ALL
def test_float32_statement(name):
    """blend() in float32 against itself in float64, per image and per moment slot in units of the slot's sum|terms|: the bars' basis.
    With every gap held, float32 takes every decision as float64 does: n_contrib is identical."""
    figs = dict(B.statement_figures(name))
    same = figs.pop("n_contrib_equal")
    _FIGURES[name] = figs
    Hh.report(f"blend/f32_statement/{name}", **figs)
    assert same == 1.0
    bad = {k: v for k, v in figs.items() if v >= 1e-3 and k != "d_tex"}       # (d_tex: see blend_ref.statement_figures; d_tex_x is held)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ windows
def _deterministic(fn):
    """fn() with torch's sequential scatter-adds: the parallel ones take duplicate indices in an order that varies from run to run,
    and bit-identity is asserted below"""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        return fn()
    finally:
        torch.use_deterministic_algorithms(was)


def _tight_windows(case):
    """per face the smallest window that holds every tap of a contributing pair"""
    R = case.R
    lo, hi = torch.full((6, 2), R), torch.full((6, 2), -1)
    with torch.no_grad():
        for tile in range(case.gx * case.gy):
            t = B._tile_forward(case, tile, case.rec.to(F64), case.texture.to(F64), F64)
            for yy, xx, _ in t.taps:
                for f in range(6):
                    m = t.contrib & (t.face == f)
                    if bool(m.any()):
                        lo[f] = torch.minimum(lo[f], torch.stack([yy[m].min(), xx[m].min()]))
                        hi[f] = torch.maximum(hi[f], torch.stack([yy[m].max(), xx[m].max()]))
    assert bool((hi >= lo).all()), "every face is reached"
    return [tuple(lo[f].tolist()) for f in range(6)], [tuple((hi[f] - lo[f] + 1).tolist()) for f in range(6)]


def test_windowed_texture_is_the_dense_texture():
    """uv_R96 three ways -- dense, as windows that cover whole faces, as the tightest windows that hold its taps: every output of the
    float64 blend() is bit-identical, the per-texel ones window by window, and the dense ones are 0 outside the tight windows.  A
    window one row short of a tap is an assertion failure, not a silent zero."""
    case = B.prepared("uv_R96").case
    R = case.R
    dense = _deterministic(lambda: B.blend(case))
    org, size = _tight_windows(case)
    assert any(h < R or w < R for h, w in size)
    covered = torch.zeros(6, R, R, dtype=torch.bool)
    for f, ((y, x), (h, w)) in enumerate(zip(org, size)):
        covered[f, y:y + h, x:x + w] = True
    assert not dense.d_tex_n[~covered].any() and not dense.d_tex[~covered].any()
    for origins, sizes in (([(0, 0)] * 6, [(R, R)] * 6), (org, size)):
        win = B.Windows.of(case.texture, origins, sizes)
        wcase = B._with(case, texture=win)
        assert wcase.R == R
        o = _deterministic(lambda: B.blend(wcase))
        for k in B.IMAGES + ("n_contrib", "color_abs", "depth_abs", "norm_abs", "pairs", "block_contrib", "M", "M_abs", "M_ext", "M_n", "d_rec"):
            assert torch.equal(getattr(o, k), getattr(dense, k)), k
        for k in ("d_tex", "d_tex_abs", "d_tex_ext", "d_tex_x", "d_tex_n"):
            for f, ((y, x), (h, w)) in enumerate(zip(origins, sizes)):
                assert torch.equal(win.face(getattr(o, k), f), getattr(dense, k)[f, y:y + h, x:x + w]), (k, f)
        gaps, off, cnt = B.decision_gaps(wcase)
        assert gaps == case.gaps and not off.any() and all(cnt[k] == case.counters[k] for k in cnt)
    short = B.Windows.of(case.texture, org, [(h - 1, w) if f == 2 else (h, w) for f, (h, w) in enumerate(size)])
    with pytest.raises(AssertionError, match="outside its face's window"):
        B.blend(B._with(case, texture=short), want_grads=False)


BIG = [n for n in B.NAMES if n.startswith("uv_big_R")]


@pytest.mark.parametrize("name", BIG)
def test_float32_statement_of_the_colour_only_pass(name):
    """the large-R cases' colour-only pass has figures of its own (blend_ref.statement_figures_colour_only), under the same cap;
    they go to profiles/blend_parity.json under "f32_statement_colour_only", where test_blend_gpu.py reads that pass's bars"""
    figs = dict(B.statement_figures_colour_only(name))
    assert figs.pop("n_contrib_equal") == 1.0
    B.store_parity("f32_statement_colour_only", {name: figs})
    Hh.report(f"blend/f32_statement_colour_only/{name}", **figs)
    bad = {k: v for k, v in figs.items() if v >= 1e-3 and k != "d_tex"}
    assert not bad, bad


def test_large_cases_are_the_ones_the_limit_promises():
    assert BIG == ["uv_big_R2368", "uv_big_R5462", "uv_big_R7168"]
    for name in BIG:
        case = B.prepared(name).case
        R, cn = case.R, case.counters
        print("BLEND CASE", name, cn)
        assert isinstance(case.texture, B.Windows) and 60 <= case.N <= 100 and (case.W, case.H) == (16, 16)
        assert case.texture.h.tolist() == [96] * 6 and case.texture.w.tolist() == [96] * 6
        assert (int(case.texture.y0[0]), int(case.texture.x0[0])) == (0, 0) and (int(case.texture.y0[5]), int(case.texture.x0[5])) == (R - 96, R - 96)
        assert all(int(v) % 32 for f in range(1, 5) for v in (case.texture.y0[f], case.texture.x0[f]))
        assert cn["bins"] > 32768 and cn["pairs_below_chunk"] >= 100 and cn["pairs_above_chunk"] >= 100
        assert min(cn["clamp_left_face0"], cn["clamp_top_face0"], cn["clamp_right_face5"], cn["clamp_bottom_face5"]) >= 10
    cn = {n: B.prepared(n).case.counters for n in BIG}
    assert cn["uv_big_R2368"]["bins"] == 32856 and cn["uv_big_R7168"]["bins"] == 301056
    assert cn["uv_big_R2368"]["last_byte_offset"] < 6 * 5461 * 5461 * 12 <= 2 ** 31 < cn["uv_big_R5462"]["last_byte_offset"]
    assert cn["uv_big_R7168"]["last_byte_offset"] == 3699376116
    for n in BIG[1:]:
        assert cn[n]["pairs_below_2_31"] >= 100 and cn[n]["pairs_above_2_31"] >= 100


@pytest.mark.parametrize("name", BIG)
def test_a_window_one_texel_off_shows(name):
    """The statement with one window's origin moved by one texel (every tap of that face reads its neighbour, every texel of its
    gradient lands one beside) against the unmoved statement: `color` and dL/dtexture in the footprint unit (d_tex_x) differ by at
    least 30 x the bars test_blend_gpu.py holds the device to -- the margin test_cubetex_gpu.test_seams_exhaustively states -- for
    each of the six windows.  Face 0's window starts at column 0 and is moved left, the others right: no tap leaves its window."""
    import test_blend_gpu as G
    p = B.prepared(name)
    case, ref = p.case, p.ref
    figs = B.statement_figures(name)
    base = {k: max(4.0 * figs[k], B.FLOOR) for k in ("color", "d_tex_x")}
    n = ref.pairs.to(F64)[None].expand_as(ref.color)
    bar_c = (base["color"] + n * B.EPS32) * ref.color_abs
    n3 = ref.d_tex_n[..., None].expand_as(ref.d_tex).to(F64)
    bar_t = (base["d_tex_x"] + n3 * B.EPS32) * ref.d_tex_x + G.REC_QUANT * ref.d_tex_x + n3 * G.REDUCE_FIXED
    ratios = {}
    for f in range(6):
        moved = B.blend(B._with(case, texture=case.texture.shifted(f, 0, -1 if f == 0 else 1)))
        assert torch.equal(moved.n_contrib, ref.n_contrib)
        dc, dt = (moved.color - ref.color).abs(), (moved.d_tex - ref.d_tex).abs()
        ratios[f] = (float((dc[bar_c > 0] / bar_c[bar_c > 0]).max()), float((dt[bar_t > 0] / bar_t[bar_t > 0]).max()))
    Hh.report(f"blend/window_shift/{name}", **{f"face{f}_{k}": v for f, r in ratios.items() for k, v in zip(("color", "d_tex_x"), r)})
    assert all(c >= 30.0 and t >= 30.0 for c, t in ratios.values()), ratios
