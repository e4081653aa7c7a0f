"""-m gpu: K6 (texgs_render_forward) and K7 + the bin reduce (texgs_backward_render) called on their own through ctypes, on the
hand-built records and tile lists of blend_ref.py: no K1 runs, no rounding precedes the kernel under test, and every discrete decision
sits clear of its threshold by construction -- no ambiguity mask, no outlier budget, no excluded row.

K6: the four images and final_T on every pixel, n_contrib identical, surv_count[b] between the Gaussians that contribute to block b in
float64 and the list length (equal to the designed count in the list-length cases), the guard words around every output untouched,
and bit-identical images with and without the hand-off pointers and under a reversed tile_order.
K7: every one of the 28 `acc` slots of every Gaussian against the moment sums of the float64 blend, rows of Gaussians in no list
exactly 0, dL_dtexture on every texel (texels outside the reference's support exactly 0) -- for want = ALL / GAUSSIANS / TEXTURE, the
record lists exactly sized / half sized / absent (atomics), and once with dL_ddepth / dL_dnorm / dL_dalpha NULL.

Bars (blend_ref.base_bar): max(4 x the float32 statement's figure of that case and output, 8 * 2^-24) in units of the output's
sum|terms|, plus n * 2^-24 for a sum of n terms taken in any order; the outputs named in EXTRA also get the derived terms written
beside the constants below, clipped at 1e-3 of the row's sum|terms| (with_extra).  The
measured figures are reported and written to profiles/blend_parity.json under "hip_vs_f64".  K7's rows are sums of float atomics from
several blocks, so a reversed tile_order is held to the same bars, not to bit-identity (K6's outputs are bit-identical).
test_records_from_k1 blends the records K1 itself wrote: the only case with an exclusion (see from_k1).
The cases uv_big_R2368 / 5462 / 7168 run the same tests at the texture sizes the ABI's limit promises (more than 32 768 texture bins,
byte offsets past 2^31) on a WindowDevice: the texture and dL_dtexture exist on the device only, between guards, and whatever K7
writes outside the six windows -- guards included -- fails the test."""
import ctypes as C

import pytest
import torch

import blend_ref as B
import helpers as Hh
import preprocess_ref as PR

pytestmark = pytest.mark.gpu

from blend_device import (  # noqa: F401  (the names other test files reach through this module too)
    F64, JUNK, Q32, TAP_ROUNDINGS, CAP, EXTRA, with_extra, REC_QUANT, REDUCE_FIXED, _FIGURES, Device,
    WindowDevice, _DEVICES, device_for, _note, _hold, _LOCAL, _case, _base, check_forward, check_backward)



@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    B.store_parity("hip_vs_f64", _FIGURES)




# ------------------------------------------------------------------------------------------------------------------ K6
@pytest.mark.parametrize("name", B.NAMES)
def test_k6_against_float64(lib_built, name):
    p, d = B.prepared(name), device_for(name)
    case = p.case
    words = d.texture_checksum()
    out, img = d.k6()
    check_forward(name, out, p.ref)
    surv = d.hand["count"].cpu().to(torch.int64).reshape(d.T, 4)
    lens = (case.ranges[:, 1] - case.ranges[:, 0])[:, None]
    assert bool((surv <= lens).all()) and bool((surv >= p.ref.block_contrib).all()), (surv, p.ref.block_contrib)
    if "survivors" in case.design:
        assert torch.equal(surv, case.design["survivors"]), (surv, case.design["survivors"])
    plain, _ = d.k6(hand_off=False)
    rev, _ = d.k6(reverse=True)
    for k in out:
        assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), ("without the hand-off pointers", k)
        assert torch.equal(out[k].view(torch.int32), rev[k].view(torch.int32)), ("reversed tile_order", k)
    assert torch.equal(surv, d.hand["count"].cpu().to(torch.int64).reshape(d.T, 4))
    assert d.texture_checksum() == words, "K6 only reads the texture"


# ------------------------------------------------------------------------------------------------------------------ K7
VARIANTS = [(3, "exact"), (3, "half"), (3, "atomics"), (2, "exact"), (1, "exact"), (1, "half"), (1, "atomics")]
# The colour-only pass of the large-R cases is held to the float32 statement OF THAT PASS (the same formula, max(4 x figure,
# 8 * 2^-24) + n * 2^-24): measured against the bars made from the full pass, as every other case's colour-only pass is, three M_P
# slots each of uv_big_R5462 (M_P 1.81 x, M_Pdydy 1.44 x, M_Pdxdx 1.32 x) and uv_big_R7168 (M_Pdx 1.90 x, M_Pdxdx 1.59 x, M_Pdy
# 1.24 x) came over on an MI355X, every other output of every flavour under (uv_big_R2368: 0.97 x at most).  The cause is in the
# statement, not in the kernel: without the depth / normal / alpha terms dL/dpower is made of colour terms alone, a colour carries
# the float32 error of its tap address (R 2^-23 texel times the step between texels), and the float32 statement of that pass stands
# at 3.8e-5 / 8.1e-5 of sum|terms| itself where the device measured 4.3e-5 / 6.8e-5 (blend_ref.statement_figures_colour_only; with
# a constant texture the statement is at 4e-7 .. 8e-7).  None of EXTRA's derived terms is that error, so none is lent to it.
COLOUR_ONLY_STATEMENT = {f"uv_big_R{R}" for R in B.BIG_RESOLUTIONS}


@pytest.mark.parametrize("name", B.NAMES)
def test_k7_against_float64(lib_built, name):
    """want = ALL / GAUSSIANS / TEXTURE x the three texture-gradient paths, then the colour-only null-pointer combination, then ALL
    again under a reversed tile_order (K7 sums a Gaussian's row with float atomics from several blocks: both orders are held to the
    bar, not to each other)"""
    p, d = B.prepared(name), device_for(name)
    case = p.case
    words = d.texture_checksum()
    _, img = d.k6()
    textured = case.texture is not None
    overflow = 0
    for want, path in VARIANTS:
        if not textured and (want == 1 or path != "exact"):
            continue
        acc, dtex, ovf = d.k7(img, want, path)
        overflow = max(overflow, ovf)
        check_backward(name, acc, dtex, p.ref, f"k7_want{want}_{path}", want, path)
        d.after_k7()
    acc, dtex, _ = d.k7(img, 3 if textured else 2, "exact", colour_only=True)
    check_backward(name, acc, dtex, B.prepared_colour_only(name), "k7_colour_only", 3 if textured else 2, "exact",
                   section="f32_statement_colour_only" if name in COLOUR_ONLY_STATEMENT else "f32_statement")
    d.after_k7()
    _, img = d.k6(reverse=True)
    acc, dtex, _ = d.k7(img, 3 if textured else 2, "exact", reverse=True)
    check_backward(name, acc, dtex, p.ref, "k7_reversed", 3 if textured else 2, "exact")
    d.after_k7()
    assert d.texture_checksum() == words, "K6 and K7 only read the texture"
    if name.startswith("uv_R"):
        assert overflow >= 10, ("overflow footprints (second half of tex_bin_count)", overflow)
        Hh.report(f"blend/hip_vs_f64/{name}/overflow_footprints", overflow=overflow)


def test_k7_nonfinite_gradient_reaches_exactly_its_support(lib_built):
    """R = 7168, one pixel's dL/dcolour = inf: the bound of the reduce's fixed-point scale is then not finite and k_texgrad_reduce
    adds every record with float atomics, rebuilding the tap's byte offset from (bin, cell) -- past bit 31 in the windows of faces 4
    and 5.  The texels that are not finite afterwards are exactly the taps of that pixel's contributing pairs in the float64
    statement (those with a colour channel above the clamp: the others pass 0 on); every other texel is held to check_backward's bars against the statement without that pixel, and nothing is written
    outside the windows.  want = TEXTURE: the moments of the pixel's Gaussians (not finite either) are not asked for."""
    name = "uv_big_R7168"
    p, d = B.prepared(name), device_for(name)
    case = p.case
    with torch.no_grad():
        t = B._tile_forward(case, 0, case.rec.to(F64), case.texture.to(F64), F64)
    pix = int(t.contrib.sum(1).argmax())
    py, px = int(t.py[pix]), int(t.px[pix])
    m = t.contrib[pix] & (t.colarg[pix] > 0).any(-1)               # (a pair whose three channels all clamp at 0 passes no gradient on, inf or not)
    assert int(m.sum()) >= 20 and int((t.contrib[pix] & ~m).sum()) >= 1
    support = torch.zeros(p.ref.d_tex_n.shape, dtype=torch.bool)
    for ix in t.tap_idx:
        support[ix[0][pix][m]] = True
    clamped = ((t.x0 < 0) | (t.x0 >= case.R - 1) | (t.y0 < 0) | (t.y0 >= case.R - 1))[pix]
    byte = (((t.face * case.R + t.y0.clamp(0, case.R - 1)) * case.R + t.x0.clamp(0, case.R - 1)) * 12)[pix]
    assert int((m & ~clamped & (byte >= 2 ** 31)).sum()) >= 3 and int((m & ~clamped & (byte < 2 ** 31)).sum()) >= 3 and int((m & clamped).sum()) >= 3
    rest = {k: v.clone() for k, v in case.up.items()}
    rest["color"][:, py, px] = 0.0
    finite = B.blend(B._with(case, up=rest))
    assert not finite.d_tex_n[~support & (p.ref.d_tex_n == 0)].any() and int(support.sum()) >= 4 * 6
    hot = case.up["color"].clone()
    hot[:, py, px] = float("inf")
    _, img = d.k6()
    was = d.up
    d.up = dict(was, color=hot.contiguous().to(d.dev))
    try:
        acc, dtex, _ = d.k7(img, 1, "exact")
    finally:
        d.up = was
    assert (int(d.cursor[d.nbins + 1]) & 0xFFFFFFFF) >= 0x7F800000, "the reduce saw a bound that is not finite"
    assert torch.equal(~torch.isfinite(dtex).all(-1), support), (int((~torch.isfinite(dtex).all(-1)).sum()), int(support.sum()))
    dtex[support] = finite.d_tex[support].to(dtex.dtype)
    check_backward(name, acc, dtex, finite, "k7_nonfinite", 1, "exact")
    d.after_k7()


# ------------------------------------------------------------------------------------------------------------------ from K1
def from_k1(flavour):
    """case i: K1 - K5 run once on the `general` scene of preprocess_ref; the fp32 records, point_list and ranges they wrote are read
    back and become the case, thr / rcull included.  These records are not ours to nudge: pairs within their bar of a threshold are
    counted (under 0.5 % of the reached pairs), and the pixels that own one are skipped -- compared on no image, and their upstream
    gradients are zero on the device and in the reference alike, so that they enter no moment and no texel."""
    name = f"from_k1_{flavour}"
    if name in _LOCAL:
        return name
    from texgs.rasterizer import GaussianRasterizationSettings, forward_raw
    pc = PR.prepared("general", flavour).case
    dev = torch.device("cuda:0")
    st = Hh.settings_for(pc.cam, pc.sh_degree, torch.zeros(3), device=dev, cls=GaussianRasterizationSettings)
    s, N = pc.scene, pc.N
    tex = B.make_texture(torch.Generator().manual_seed(9000), 40) if flavour == "textured" else None
    t = lambda x: None if x is None else x.to(dev)
    _, state = forward_raw(st, t(s.means3D), t(s.shs), t(s.opacities), t(s.scales), t(s.rotations), t(s.uvs), t(s.gradient_uvs), t(tex),
                           color_offset=t(s.color_offset))
    torch.cuda.synchronize()
    rt, rs = state.tensors["rec"][:N].cpu().clone(), state.tensors["rec_shade"][:N].cpu().clone()
    pl = state.tensors["point_list"][:state.D].cpu().to(torch.int64)
    ranges = state.tensors["ranges"].cpu().to(torch.int64).reshape(-1, 2) & 0xFFFFFFFF
    listed = torch.zeros(N, dtype=torch.bool)
    listed[pl] = True
    rec = torch.cat([rt[:, 0:2], -2.0 * rt[:, 2:3], -rt[:, 3:4], -2.0 * rt[:, 4:5], rt[:, 5:6], rs[:, 0:18]], 1)
    assert bool(torch.isfinite(rec[listed]).all()) and int(listed.sum()) >= 200         # (about a fifth of the scene's box lies in the frustum)
    rec[~listed] = 0.0                                   # culled rows: whatever the buffers held, never read
    case = B.Case(name, PR.W, PR.H, rec, pl, ranges, tex, 9001)
    thr, rcull = rt[:, 7].clone(), rt[:, 6].clone()
    thr[~listed], rcull[~listed] = 1.0, -1.0
    case.cull = (thr, rcull)
    worst, _, cnt = B.decision_gaps(case)
    assert cnt["bad_pairs"] < 0.005 * cnt["reached"], (cnt["bad_pairs"], cnt["reached"])
    for v in case.up.values():
        v[:, case.bad_pixels] = 0.0
    Hh.report(f"blend/hip_vs_f64/{name}/excluded", bad_pairs=cnt["bad_pairs"], reached_pairs=cnt["reached"],
              skipped_pixels=int(case.bad_pixels.sum()), pixels=case.W * case.H)
    ref, f32 = B.blend(case), B.blend_f32(case)
    figs = {}
    keep = ~case.bad_pixels
    for k in ("color", "depth", "norm", "alpha", "final_T"):
        unit = {"alpha": ref.alpha, "final_T": ref.final_T}.get(k, getattr(ref, k + "_abs", None))
        m = keep.expand_as(getattr(ref, k))
        figs[k] = B.unit_error(getattr(f32, k)[m], getattr(ref, k)[m], unit[m])
    for i, nm in enumerate(B.MOMENT_NAMES):
        figs["M_" + nm] = B.unit_error(f32.M[:, i], ref.M[:, i], ref.M_abs[:, i])
    if tex is not None:
        figs["d_tex"], figs["d_tex_x"] = B.unit_error(f32.d_tex, ref.d_tex, ref.d_tex_abs), B.unit_error(f32.d_tex, ref.d_tex, ref.d_tex_x)
    B.store_parity("f32_statement", {name: figs})
    Hh.report(f"blend/f32_statement/{name}", **figs)
    _LOCAL[name] = (case, figs, ref)
    return name


@pytest.mark.parametrize("flavour", ["textured", "coff"])
def test_records_from_k1(lib_built, flavour):
    """ties the hand-built convention to what K1 really writes: K6 and K7 (want = ALL, exact lists) on K1's own fp32 records"""
    name = from_k1(flavour)
    case, _, ref = _LOCAL[name]
    d = Device(case)
    out, img = d.k6()
    check_forward(name, out, ref, skip=case.bad_pixels)
    want = 3 if case.texture is not None else 2
    acc, dtex, _ = d.k7(img, want, "exact")
    check_backward(name, acc, dtex, ref, f"k7_want{want}_exact", want, "exact")
