"""K6 / K7 alone, on the CPU: the float64 statement of blend_ref.py agrees with oracle.texgs_torch.render + autograd to 1e-10 (images,
final_T, the record and texture gradients; n_contrib identical), its moment sums turn into autograd's dL/d(record) through
preprocess_ref.cotangent_from_moments to 1e-10 (the M_* definitions of csrc/common.h, pinned a second way), every builder holds its
floors and gaps, and the same statement evaluated in float32 -- the basis of the bars of test_blend_gpu.py -- takes every decision
as float64 does.  The float32 figures go to profiles/blend_parity.json under "f32_statement"."""
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
    figs = B.statement_figures(name)
    same = figs.pop("n_contrib_equal")
    _FIGURES[name] = figs
    Hh.report(f"blend/f32_statement/{name}", **figs)
    assert same == 1.0
    bad = {k: v for k, v in figs.items() if v >= 1e-3 and k != "d_tex"}       # (d_tex: see blend_ref.statement_figures; d_tex_x is held)
    assert not bad, bad
