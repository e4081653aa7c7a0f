"""-m gpu: the order of K7's segment pipeline (csrc/render_bwd_body.h) -- stage C of segment n - 1 runs inside the waits of stage B of
segment n, L.items holds the previous segment until the back half writes the new one, and C of a chunk's last segment runs at the
chunk's end.  K7 on its own (texgs_backward_render on the state one K6 call left, as in test_blend_gpu.py), on hand-built single-tile
cases of 16x16 pixels made with blend_ref's builders, against blend_ref.blend in float64, for the full (want = ALL), the
frozen-texture (want = GAUSSIANS, textured) and the untextured flavour -- the three that have a stage C.

Every case is named for a shape of the walk of block 0 (the tile's first 8x8 block): how many segments a chunk has, what closed a
segment, how many tasks stage C2 finds in it, where a chunk ends.  walk() replays that control flow on the CPU from the float64
blend's contributor table: K6's survivors and quadrant masks from a float64 port of block_reachable (no answer changes when every
comparison moves by 1e-3, asserted), chunks of 64 survivors from the back, one list per 4x4 quadrant, lock-step iterations, a segment closed
by the 64-item cap (the cut iteration is tested again), by BWD_MAX_IT = 16 productive iterations or by the end of the lists.  The
counts each case is built for are asserted from that walk before anything runs, and the survivor list the walk assumed is compared
with the one K6 handed to K7.

Bars: test_k7_against_float64's rule, applied here by ratios() -- every output is held to the bare bar max(4 x the float32 statement's
figure of the case and output, 8 * 2^-24) + n * 2^-24 in units of the output's sum|terms| (the texture gradient also carries the record
format's quantisation); only the outputs that EXTRA names, because they were measured over that bar on an MI355X, get the derived term
of blend_ref (PAIR_ROUNDINGS / W_STEPS / P_STEPS) beside it, clipped at 1e-3 of the row's sum|terms|.  Of the 33 runs one case is named:
the untextured 129-survivor list, seven w-linear outputs, worst 1.35 x bare."""
import functools
from types import SimpleNamespace

import pytest
import torch

import blend_ref as B
import helpers as Hh
import test_blend_gpu as TB

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
BQ_CAP, BWD_MAX_IT = 64, 16
R_TEX = 32
CLEAR = 1e-3                       # no answer of the cull port changes when every comparison moves by this much (pixels / units of power)


# ------------------------------------------------------------------------------------------------------------------ the walk
def _reach(rec, thr, rcull, x0, y0, ext, slack=0.0):
    """block_reachable (render.hip) in float64, every comparison loosened by `slack` (tightened by a negative one) -> bool [N]"""
    gx, gy = rec[:, 0], rec[:, 1]
    ah, bh, ch = -0.5 * rec[:, 2], -rec[:, 3], -0.5 * rec[:, 4]
    x1, y1 = x0 + ext, y0 + ext
    in_disc = (rcull >= 0) & (gx + rcull >= x0 - slack) & (gx - rcull <= x1 + slack) & (gy + rcull >= y0 - slack) & (gy - rcull <= y1 + slack)
    dx0, dx1, dy0, dy1 = gx - x1, gx - x0, gy - y1, gy - y0
    centre = (dx0 <= slack) & (dx1 >= -slack) & (dy0 <= slack) & (dy1 >= -slack)

    def edge_x(dx):
        dy = torch.minimum(dy1, torch.maximum(dy0, bh * dx * (-0.5 / ch)))
        return ah * dx * dx + bh * dx * dy + ch * dy * dy

    def edge_y(dy):
        dx = torch.minimum(dx1, torch.maximum(dx0, bh * dy * (-0.5 / ah)))
        return ah * dx * dx + bh * dx * dy + ch * dy * dy

    best = torch.maximum(torch.maximum(edge_x(dx0), edge_x(dx1)), torch.maximum(edge_y(dy0), edge_y(dy1)))
    return in_disc & (centre | (best >= thr - 1e-3 * thr.abs() - 1e-4 - slack))


def _reach_clear(case, rec, thr, rcull, x0, y0, ext):
    """the cull's answer, asserted to be the same with every comparison moved by CLEAR either way"""
    r = _reach(rec, thr, rcull, x0, y0, ext)
    assert torch.equal(r, _reach(rec, thr, rcull, x0, y0, ext, CLEAR)) and torch.equal(r, _reach(rec, thr, rcull, x0, y0, ext, -CLEAR)), \
        (case.name, "a cull decision within", CLEAR, "of its threshold")
    return r


def walk(case, block=0):
    """K7's control flow over 8x8 block `block` of tile 0 -> namespace: survivors (list positions, ascending), qmask [survivor][4],
    chunks: per chunk of the walk (from the back) either "skipped" or the list of its segments, each dict(items, iters, tasks, closed)
    with closed in {"cap", "max_it", "end"}"""
    rec = case.rec.to(F64)
    with torch.no_grad():
        t = B._tile_forward(case, 0, rec, None if case.texture is None else case.texture.to(F64), F64)
    thr, rcull = (v.to(F64) for v in B.cull_aids(case.rec))
    ids = t.ids
    bx, by = 8.0 * (block % 2), 8.0 * (block // 2)
    reach = _reach_clear(case, rec[ids], thr[ids], rcull[ids], bx, by, 7.0)
    qm = [_reach_clear(case, rec[ids], thr[ids], rcull[ids], bx + 4.0 * (q % 2), by + 4.0 * (q // 2), 3.0) for q in range(4)]
    qm = torch.stack(qm, 1)
    surv = [int(p) for p in torch.nonzero(reach).reshape(-1)]
    todo = t.K
    pix = [(t.block == block) & (t.quad == q) for q in range(4)]
    cnt = torch.stack([t.contrib[pix[q]].sum(0) for q in range(4)], 1)            # [K,4] contributing pixels per list entry and quadrant
    # K6 culls on as long as a pixel of the block is alive: every case here keeps one (asserted), so every reachable entry is handed over
    assert float(t.Tfin[(t.block == block) & t.inside].max()) >= B.T_EPS
    rowlast = [min(int(t.n_contrib[pix[q]].max()), todo) for q in range(4)]
    wave_last = max(rowlast)
    chunks = []
    for hi in range(len(surv), 0, -64):
        chunk = surv[max(0, hi - 64):hi][::-1]
        if chunk[-1] >= wave_last:
            chunks.append("skipped")
            continue
        lists = [[p for p in chunk if bool(qm[p, q]) and p < rowlast[q]] for q in range(4)]
        tmax = max(len(l) for l in lists)
        ti, segs = 0, []
        while True:
            seg = dict(items=0, iters=0, tasks=0, closed="end")
            while ti < tmax and seg["iters"] < BWD_MAX_IT:
                c = [int(cnt[lists[q][ti], q]) if ti < len(lists[q]) else 0 for q in range(4)]
                if sum(c) > 0:
                    if seg["items"] + sum(c) > BQ_CAP:
                        seg["closed"] = "cap"                    # this iteration is tested again in the next segment
                        break
                    seg["items"] += sum(c)
                    seg["iters"] += 1
                    seg["tasks"] += sum(1 for v in c if v > 0)
                ti += 1
            if seg["closed"] == "end" and seg["iters"] == BWD_MAX_IT and ti < tmax:
                seg["closed"] = "max_it"
            if seg["items"] == 0:
                break
            segs.append(seg)
            if ti >= tmax:
                break
        chunks.append(segs)
    return SimpleNamespace(survivors=surv, qmask=qm, chunks=chunks, wave_last=wave_last, contrib=cnt)


# ------------------------------------------------------------------------------------------------------------------ builders
def _splat(g, kind):
    """one record row.  W: wide, all 64 pixels of every block.  Confined to quadrant 0 of block 0 (pixels 0..3 x 0..3, nothing beyond
    reachable): F sigma 1 at the quadrant's centre, all 16 pixels; S sigma 0.5 between four pixels, those four; O sigma 0.35 on a
    pixel (a few hundredths off it), that one.  X: near-opaque, sigma 3 at the quadrant's centre -- a dozen of them finish all 16 pixels of the quadrant."""
    u = lambda *s: torch.rand(*s, generator=g)
    if kind == "W":
        return B._wide(g, 1)
    r = B._rec(1)
    if kind == "F":
        r[0, 0:2] = 1.45 + 0.1 * u(2)
        r[0, 2] = r[0, 4] = 1.0
        r[0, 5] = 0.05 + 0.02 * u(1)
    elif kind == "S":
        r[0, 0:2] = torch.randint(0, 3, (2,), generator=g).to(F32) + 0.5
        r[0, 2] = r[0, 4] = 4.0
        r[0, 5] = 0.027 + 0.004 * u(1)
    elif kind == "O":
        off = (0.02 + 0.03 * u(2)) * (2.0 * torch.randint(0, 2, (2,), generator=g).to(F32) - 1.0)      # (never on a rectangle's edge)
        r[0, 0:2] = torch.randint(0, 4, (2,), generator=g).to(F32) + off
        r[0, 2] = r[0, 4] = 8.0
        r[0, 5] = 0.025 + 0.01 * u(1)
    elif kind == "X":
        r[0, 0:2] = 1.4 + 0.2 * u(2)
        r[0, 2] = r[0, 4] = 1.0 / 9.0
        r[0, 5] = 0.88 + 0.07 * u(1)
    else:
        raise ValueError(kind)
    return r


# the list entries in the order K7 walks them (back to front: the first letter is the LAST list entry)
WALKS = {
    "seg1": "W",
    "seg2": "WW",
    "seg3": "WWW",
    "max_it": "O" * 20,
    "last_one_item": "O" * 17,
    "cap_retest": "FFFFFS",
    "tasks5": "FFFSSF",
    "tasks9": "FFFOOOOOOFO",
    "surv65": ("FSOSO" * 13)[:64] + "W",
    "surv129": ("OSFWS" * 26)[:128] + "F",
    "skipped_chunk": ("SOF" * 23)[:68] + "X" * 12 + "FSOW" * 5,
}
FLAVOURS = {"full": (True, 3), "frozen_texture": (True, 2), "untextured": (False, 2)}


def _segs(w):
    return [[(s["items"], s["iters"], s["tasks"], s["closed"]) for s in c] if c != "skipped" else c for c in w.chunks]


def _expect(name, w):
    """the property the case is named for, from the reference walk"""
    s = _segs(w)
    flat = [x for c in s if c != "skipped" for x in c]
    if name in ("seg1", "seg2", "seg3"):
        k = int(name[3])
        assert s == [[(64, 1, 4, "cap")] * (k - 1) + [(64, 1, 4, "end")]], s
    elif name == "max_it":
        assert s == [[(16, 16, 16, "max_it"), (4, 4, 4, "end")]], s
    elif name == "last_one_item":
        assert s == [[(16, 16, 16, "max_it"), (1, 1, 1, "end")]], s
    elif name == "cap_retest":
        assert s == [[(64, 4, 4, "cap"), (20, 2, 2, "end")]], s
    elif name == "tasks5":
        assert s == [[(56, 5, 5, "cap"), (16, 1, 1, "end")]], s
    elif name == "tasks9":
        assert s == [[(54, 9, 9, "cap"), (17, 2, 2, "end")]], s
    elif name in ("surv65", "surv129"):
        n = int(name[4:])
        assert len(w.survivors) == n and all(c != "skipped" for c in s), s
        assert len(s) == (n + 63) // 64 and len(s[-1]) == 1 and all(len(c) >= 2 for c in s[:-1]), s      # one survivor left for the last chunk
        assert {x[3] for x in flat} >= {"cap", "end"}, s
        if n == 129:
            assert s[-1] == [(16, 1, 1, "end")], s
        else:
            assert s[-1] == [(64, 1, 4, "end")], s
    elif name == "skipped_chunk":
        assert len(w.survivors) == 100 and w.wave_last <= 36, (len(w.survivors), w.wave_last)
        # (a chunk is skipped when its lowest position lies behind the last contributor, and positions fall from chunk to chunk: the
        #  skipped chunks are always the FIRST of the walk.  No case can put a `continue` behind a chunk that produced items, and the
        #  kernel has nothing pending there anyway -- stage C of a chunk's last segment runs at that chunk's end.  This case covers a
        #  skipped chunk followed by a producing one, nothing more.)
        assert s[0] == "skipped" and s[1] != "skipped" and len(s) == 2 and sum(x[0] for x in s[1]) >= 64, s
    assert all(1 <= x[0] <= BQ_CAP and 1 <= x[1] <= BWD_MAX_IT for x in flat), s


@functools.lru_cache(maxsize=None)
def prepared(name, textured):
    """the case, its float64 blend, the float32 statement's figures (the basis of the bars) and the walk -- once per process"""
    seed = 7000 + 16 * sorted(WALKS).index(name) + (0 if textured else 1)
    g = torch.Generator().manual_seed(seed)
    kinds = WALKS[name][::-1]                                    # list order, front to back
    r = torch.cat([_splat(g, k) for k in kinds], 0)
    n = r.shape[0]
    B._fill_common(g, r, textured)
    if textured:
        u = lambda *s: torch.rand(*s, generator=g)
        B._uv_plane(g, r, R_TEX, torch.randint(0, 6, (n,), generator=g), 4.0 + 24.0 * u(n), 4.0 + 24.0 * u(n), 0.1 + 0.2 * u(n))
    case = B._single_tile(f"k7order_{name}" + ("" if textured else "_untex"), r, B.make_texture(g, R_TEX) if textured else None, seed)
    assert case.W == 16 and case.H == 16 and case.R <= 40
    B.settle(case, seed)
    w = walk(case)
    _expect(name, w)
    ref, f32 = B.blend(case), B.blend_f32(case)
    figs = {"M_" + nm: B.unit_error(f32.M[:, i], ref.M[:, i], ref.M_abs[:, i]) for i, nm in enumerate(B.MOMENT_NAMES)}
    if textured:
        figs["d_tex"], figs["d_tex_x"] = B.unit_error(f32.d_tex, ref.d_tex, ref.d_tex_abs), B.unit_error(f32.d_tex, ref.d_tex, ref.d_tex_x)
    return SimpleNamespace(case=case, ref=ref, figs=figs, walk=w)


def test_task_counts_covered():
    """segments with 1, 4, 5 and 9 tasks exist among the cases (one, one, two and three rounds of stage C2)"""
    seen = set()
    for name in WALKS:
        for c in prepared(name, True).walk.chunks:
            if c != "skipped":
                seen |= {s["tasks"] for s in c}
    assert {1, 4, 5, 9} <= seen, sorted(seen)


# Outputs measured over their bare bar on an MI355X (three runs of every case and flavour with no derived term at all, the worst of
# them, named when it came above 0.99 of the bare bar as in test_blend_gpu.EXTRA): only these get the derived term written beside
# them, clipped at 1e-3 of the row's sum|terms|.  Every other output of every case is held to the bare bar.
EXTRA = {k: set(v.split()) for k, v in {
    # worst 1.35 x bare (M_vd0), 0.036 of the bar with the term: the w-linear moments of a pixel that 129 list entries reach -- every
    # term carries the roundings of the transmittance chain T <- T * rcp(1 - alpha) walked back over all of them (W_STEPS per entry)
    "k7order_surv129_untex": "M_vd0 M_vd1 M_vd2 M_depth M_n0 M_n1 M_n2",
}.items()}


def ratios(p, acc, dtex, want):
    """test_blend_gpu.check_backward's comparison (record lists exactly sized) on a case of this file -> {output: (error / bare bar,
    error / (bare bar + derived term, clipped))}, the bare bar max(4 x float32 statement, 8 * 2^-24) + n * 2^-24 in units of the row's
    sum|terms| (+ the record format's quantisation on the texture gradient, which the record lists always carry)"""
    case, ref, out = p.case, p.ref, {}
    base = lambda k: max(4.0 * p.figs[k], B.FLOOR)
    worst = lambda d, bar: float((d[bar > 0] / bar[bar > 0]).max()) if bool((bar > 0).any()) else 0.0
    ext_bar = lambda bare, ext, unit: torch.minimum(bare + ext, torch.maximum(bare, TB.CAP * unit))
    assert bool(torch.isfinite(acc).all())
    assert not acc[~case.in_lists()].any(), "rows of Gaussians that are in no list stay exactly 0"
    assert not acc[:, 28:].any()
    if case.texture is None:
        assert not acc[:, B.UV_SLOTS].any(), "untextured: the UV slots of acc stay exactly 0"
    for s, nm in enumerate(B.MOMENT_NAMES):
        unit = ref.M_abs[:, s]
        bare = (base("M_" + nm) + ref.M_n.to(F64) * B.EPS32) * unit
        d = (acc[:, s].to(F64) - ref.M[:, s]).abs()
        assert not d[bare == 0].any(), nm
        out["M_" + nm] = (worst(d, bare), worst(d, ext_bar(bare, B.EPS32 * ref.M_ext[:, s], unit)))
    if dtex is not None:
        if want & 1:
            assert bool(torch.isfinite(dtex).all())
            assert not dtex[ref.d_tex_n == 0].any(), "texels outside the reference's support stay exactly 0"
            n3 = ref.d_tex_n[..., None].expand_as(ref.d_tex).to(F64)
            d = (dtex.to(F64) - ref.d_tex).abs()
            quant = TB.REC_QUANT * ref.d_tex_x + n3 * TB.REDUCE_FIXED
            ext = TB.TAP_ROUNDINGS * case.R * B.EPS32 * ref.d_tex_x + B.EPS32 * ref.d_tex_ext
            for k, unit in (("d_tex", ref.d_tex_abs), ("d_tex_x", ref.d_tex_x)):
                bare = (base(k) + n3 * B.EPS32) * unit
                out[k] = (worst(d, bare + quant), worst(d, ext_bar(bare, ext, ref.d_tex_x) + quant))
        else:
            assert not dtex.any(), "without WANT_TEXTURE dL_dtexture is not touched"
    return out


_DEVICES = {}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", list(WALKS))
def test_k7_segment_order(lib_built, name, flavour):
    textured, want = FLAVOURS[flavour]
    p = prepared(name, textured)
    case, w = p.case, p.walk
    if case.name not in _DEVICES:
        _DEVICES[case.name] = TB.Device(case)
    d = _DEVICES[case.name]
    _, img = d.k6()
    # the survivor list the walk assumed is the one K7 gets (block 0 of tile 0: the hand-off's first entries)
    ns = int(d.hand["count"].cpu()[0])
    sv = d.hand["survivors"].cpu().to(torch.int64).reshape(-1, 2)[:ns, 1]
    qm = d.hand["qmask"].cpu().to(torch.int64)[:ns] & 15
    assert sv.tolist() == w.survivors, (sv.tolist(), w.survivors)
    want_qm = (w.qmask[w.survivors].to(torch.int64) * torch.tensor([1, 2, 4, 8])).sum(1)
    assert torch.equal(qm, want_qm), (qm, want_qm)
    acc, dtex, _ = d.k7(img, want, "exact")
    r = ratios(p, acc, dtex, want)
    named = EXTRA.get(case.name, ())
    over = {k: (ext if k in named else bare) for k, (bare, ext) in r.items()}
    Hh.report(f"k7order/over_bare_bar/{case.name}/{flavour}", **{k: v[0] for k, v in r.items()})
    bad = {k: v for k, v in over.items() if not v <= 1.0}
    assert not bad, (case.name, flavour, bad)
