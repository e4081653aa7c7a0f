"""-m gpu: K1 (texgs_preprocess_forward) and K8 (texgs_backward_preprocess) called on their own through ctypes, on the scenes of
preprocess_ref.py.  K1: radii / rect / tiles_touched bit-equal to the C oracle, every record field against float64, thr / rcull against
their formulas, culled rows.  K8: `acc` holds the f32 moment rows of moments_from_pairs; every per-Gaussian output against float64
autograd on every visible row, culled rows exactly zero, the visible rows of `acc` handed back zeroed; the COV, colour-offset and DEFER
(+ texgs_sh_flush) flavours and the `accumulate` / `want` masks.

Bar, per regime, flavour and output: max(4 x the C oracle's figure in profiles/preprocess_parity.json, 8 * 2^-24) on the row metric
max|d| / (max|row| + 1e-4 max|all|) -- no outlier budget, no excluded row (preprocess_ref.hip_bar).  The measured figures are
reported and written beside the C oracle's under "hip_vs_f64"."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import preprocess_ref as PR
from oracle import texgs_ref as CR

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("regime,flavour", PR.ALL_CASES, ids=[f"{r}-{f}" for r, f in PR.ALL_CASES])
SIZE_CASES = [f"size_{n}" for n in PR.SIZES]
SH_CASES = [f"sh_K{K}_deg{d}" for K, d in PR.SH_CASES]
OUT_SHAPE = {"means3D": 3, "means2D": 3, "opacities": 1, "scales": 3, "rotations": 4, "uvs": 3, "color_offset": 3, "cov3D": 6}
ACC_ALL = 511
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    PR.store_parity("hip_vs_f64", _FIGURES)


def _check(case, variant, figures):
    """report, record (the worst figure of an output over the variants of a case) and hold every figure to its bar"""
    Hh.report(f"preprocess/hip_vs_f64/{case.name}/{case.flavour}/{variant}", **figures)
    rec = _FIGURES.setdefault(case.name, {}).setdefault(case.flavour, {})
    for k, v in figures.items():
        rec[k] = max(rec.get(k, 0.0), v)
    for k, v in figures.items():
        bar = PR.hip_bar(case.name, case.flavour, k)
        assert v <= bar, (case.name, case.flavour, variant, k, v, bar)


class Device:
    """One case on the GPU: its inputs, the frame, K1's state."""

    def __init__(self, case):
        from texgs import _lib
        self.L, self.lib, self.case = _lib, _lib.load(), case
        self.dev = dev = torch.device("cuda:0")
        s, st = case.scene, case.settings()
        N, K = case.N, case.K
        up = lambda t: None if t is None else t.to(torch.float32).contiguous().to(dev)
        self.t = {n: up(getattr(s, n)) for n in ("means3D", "shs", "scales", "rotations", "uvs", "gradient_uvs", "texture", "color_offset",
                                                 "cov3D_precomp")}
        self.t["opacities"] = up(s.opacities.reshape(-1))
        self.cam = {n: up(v) for n, v in (("bg", st.bg), ("V", st.viewmatrix), ("P", st.projmatrix), ("campos", st.campos))}
        p = _lib.ptr
        self.frame = _lib.Frame(st.image_height, st.image_width, st.tanfovx, st.tanfovy, st.scale_modifier, st.sh_degree, K, 4, N, 0,
                                p(self.cam["bg"]), p(self.cam["V"]), p(self.cam["P"]), p(self.cam["campos"]))
        self.inputs = _lib.Inputs(*[p(self.t[n]) for n in ("means3D", "shs", "opacities", "scales", "rotations", "uvs", "gradient_uvs",
                                                             "texture", "color_offset", "cov3D_precomp")])
        nbytes = int(self.lib.texgs_scan_temp_bytes(N))
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
        self.g = dict(rec_test=torch.full((N, _lib.REC_TEST_FLOATS), float("nan"), device=dev),
                      rec_shade=torch.full((N, _lib.REC_SHADE_FLOATS), float("nan"), device=dev), depth=z(N),
                      radii=torch.full((N,), -7, dtype=torch.int32, device=dev), rect=z(N, 2, dt=torch.int32),
                      tiles=torch.full((N,), -7, dtype=torch.int32, device=dev), offsets=z(N, dt=torch.int32),
                      scan=z(nbytes + 16, dt=torch.uint8))
        g = self.g
        self.geom = _lib.Geom(p(g["rec_test"]), p(g["rec_shade"]), p(g["depth"]), p(g["radii"]), p(g["rect"]), p(g["tiles"]), p(g["offsets"]),
                              p(g["scan"]), nbytes)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def k1(self):
        self.L.call(self.lib.texgs_preprocess_forward, C.byref(self.frame), C.byref(self.inputs), C.byref(self.geom), self.stream)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in self.g.items() if k != "scan"}

    def outputs(self, fill, shs_offset=0):
        """the per-Gaussian output buffers of the flavour, filled by fill(name, shape) (a CPU float32 tensor); dL/dshs starts
        `shs_offset` floats into its allocation (1: sh_rows_out's scalar path)"""
        c = self.case
        out = {n: fill(n, (c.N, OUT_SHAPE[n])).to(self.dev) for n in PR.INPUTS[c.flavour] if n != "shs"}
        self._shs_alloc = torch.zeros(c.N * c.K * 3 + 4, device=self.dev)
        out["shs"] = self._shs_alloc[shs_offset:shs_offset + c.N * c.K * 3].view(c.N, c.K, 3)
        out["shs"].copy_(fill("shs", (c.N, c.K, 3)).to(self.dev))
        assert out["shs"].data_ptr() % 16 == 4 * shs_offset
        return out

    def k8(self, M32, out, accumulate=0, want=2, residue=None):
        """-> (outputs on the CPU, acc on return)"""
        p = self.L.ptr
        acc = M32.to(self.dev).contiguous()
        gr = self.L.Grads()
        gr.acc, gr.want, gr.accumulate = p(acc), want, accumulate
        gr.dL_dmeans3D, gr.dL_dmeans2D, gr.dL_dshs, gr.dL_dopacities = p(out["means3D"]), p(out["means2D"]), p(out["shs"]), p(out["opacities"])
        gr.dL_dscales, gr.dL_drotations, gr.dL_duvs = p(out.get("scales")), p(out.get("rotations")), p(out.get("uvs"))
        gr.dL_dcolor_offset, gr.dL_dcov3D, gr.dL_dvd_residue = p(out.get("color_offset")), p(out.get("cov3D")), p(residue)
        self.L.call(self.lib.texgs_backward_preprocess, C.byref(self.frame), C.byref(self.inputs), C.byref(self.geom), C.byref(gr), self.stream)
        torch.cuda.synchronize()
        return {n: v.cpu() for n, v in out.items()}, acc.cpu()

    def flush(self, out, residue):
        from texgs.multiview import ShFlushView, sh_flush_entry
        c, p = self.case, self.L.ptr
        views = (ShFlushView * 1)(ShFlushView(p(self.cam["campos"]), p(residue), c.sh_degree, c.K))
        self.L.call(sh_flush_entry(), c.N, c.K, p(self.t["means3D"]), p(self.t["shs"]), p(out["shs"]), p(out["means3D"]), views, 1, self.stream)
        torch.cuda.synchronize()
        return {n: v.cpu() for n, v in out.items()}


_DEVICES = {}


def device_for(regime, flavour="textured"):
    """the case on the GPU with K1 already run (K8 reads its radii); one per case and process"""
    key = (regime, flavour)
    if key not in _DEVICES:
        d = Device(PR.prepared(regime, flavour).case)
        d.state = d.k1()
        _DEVICES[key] = d
    return _DEVICES[key]


def nan_fill(name, shape):
    return torch.full(shape, float("nan"))


def random_fill(p, seed):
    """start values of the size of the gradient they will be added to (row by row; 1e-3 of the largest entry where the row has
    none), so that an output added into instead of overwritten, or the reverse, is an error of the order of the row itself"""
    g = torch.Generator().manual_seed(seed)

    def fill(name, shape):
        ref = p.ref[name].reshape(shape[0], -1).abs()
        size = ref.max(1, keepdim=True).values + 1e-3 * ref.max().clamp_min(1e-3)
        return (torch.randn(shape[0], ref.shape[1], generator=g, dtype=PR.F64) * size).to(torch.float32).reshape(shape)
    return fill


def _reshape(p, n, t):
    return t.reshape(p.ref[n].shape)


# ------------------------------------------------------------------------------------------------------------------ K1
@CASES
def test_k1_integer_state_and_culled_rows(lib_built, regime, flavour):
    """radii, rect, tiles_touched bit-equal to the C oracle; culled rows: radii 0, tiles_touched 0, depth key 0xFFFFFFFF; depth keys of
    the visible rows bit-equal too"""
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    N, s = p.case.N, d.state
    ref = CR.RefRun(p.case.scene, p.case.settings())
    ref.forward()
    vis = ref.radii[:N] > 0
    assert np.array_equal(vis, p.visible.numpy())
    assert np.array_equal(s["radii"].numpy(), ref.radii[:N])
    assert np.array_equal(s["tiles"].numpy().astype(np.uint32), ref.tiles[:N])
    rect = s["rect"].numpy().astype(np.uint32)
    got = np.stack([rect[:, 0] & 0xFFFF, rect[:, 0] >> 16, rect[:, 1] & 0xFFFF, rect[:, 1] >> 16], 1).astype(np.int32)
    assert np.array_equal(got[vis], ref.rect[:N][vis])
    depth = s["depth"].numpy().view(np.uint32)
    assert np.array_equal(depth[vis], ref.depth[:N][vis].view(np.uint32))
    assert np.all(depth[~vis] == 0xFFFFFFFF) and not s["radii"].numpy()[~vis].any() and not s["tiles"].numpy()[~vis].any()
    assert not rect[~vis].any()


@CASES
def test_k1_records(lib_built, regime, flavour):
    """rec_test / rec_shade against record64 in the layout K1 writes: xy, conic pre-scaled by (-1/2, -1, -1/2), opacity, rcull, thr |
    g, G, phi ((0, 0, 1) without a texture), viewdep, depth, normal, xy again.  thr = -ln(255 op) - 1e-3 (1 for op = 0, where nothing
    can pass) and rcull = 1.001 sqrt(-2 thr lam) + 0.01 (-1 where thr >= 0), lam the larger eigenvalue of cov2D, in float64: thr to a
    few fp32 roundings of max(1, |thr|) (logf), rcull to the bar of the conic it is made from plus those roundings."""
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    case, v = p.case, p.visible
    rt, rs = d.state["rec_test"].to(PR.F64), d.state["rec_shade"].to(PR.F64)
    assert bool(torch.isfinite(rt[v]).all()) and bool(torch.isfinite(rs[v]).all())
    got = torch.cat([rt[:, 0:2], rt[:, 2:3] / -0.5, rt[:, 3:4] / -1.0, rt[:, 4:5] / -0.5, rt[:, 5:6], rs[:, 0:18]], 1)
    _check(case, "k1", {f"rec_{k}": PR.row_error(got[:, a:b], p.rec[:, a:b], v) for k, (a, b) in PR.FIELDS.items()})
    assert torch.equal(d.state["rec_shade"][v][:, 18:20], d.state["rec_test"][v][:, 0:2])
    if not case.textured:
        assert torch.equal(d.state["rec_shade"][v][:, 8:11], torch.tensor([0.0, 0.0, 1.0]).expand(int(v.sum()), 3))
    op = p.rec[v][:, PR.R_OP]
    con = p.rec[v][:, PR.R_CONIC:PR.R_CONIC + 3]
    det = 1.0 / (con[:, 0] * con[:, 2] - con[:, 1] ** 2)
    mid = 0.5 * (con[:, 2] * det + con[:, 0] * det)
    lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    thr = torch.where(op > 0, -torch.log(255.0 * torch.where(op > 0, op, torch.ones_like(op))) - 1e-3, torch.ones_like(op))
    rcull = torch.where(thr < 0, torch.sqrt((-2.0 * thr * lam).clamp_min(0.0)) * 1.001 + 0.01, -torch.ones_like(op))
    thr_err = float(((rt[v][:, 7] - thr).abs() / thr.abs().clamp_min(1.0)).max())
    rcull_err = float(((rt[v][:, 6] - rcull).abs() / rcull.abs().clamp_min(1.0)).max())
    Hh.report(f"preprocess/hip_vs_f64/{case.name}/{flavour}/k1_cull_aids", thr=thr_err, rcull=rcull_err)
    assert thr_err <= PR.FLOOR, thr_err
    # thr enters under the root beside lam; near thr = 0 its own rounding (relative to max(1, |thr|)) is amplified by 1 / |thr|
    slack = PR.FLOOR * float((1.0 / thr.abs().clamp_min(1e-3)).clamp_min(1.0).max()) if bool((thr < 0).any()) else 0.0
    assert rcull_err <= PR.hip_bar(case.name, flavour, "rec_conic") + PR.FLOOR + slack, (rcull_err, slack)


# ------------------------------------------------------------------------------------------------------------------ K8
def _compare(p, got, acc, variant, start=None):
    """every output against float64 on every visible row, within its bar.  `start` {name: CPU tensor}: the values K8 (or the flush)
    ADDED the gradient to -- the expectation is their sum, and the start value joins the row's denominator (preprocess_ref.row_error)"""
    case, v = p.case, p.visible
    start = start or {}
    figs = {}
    for n in PR.INPUTS[case.flavour]:
        s0 = start[n].to(PR.F64).reshape(p.ref[n].shape) if n in start else None
        figs[n] = PR.row_error(_reshape(p, n, got[n]), p.ref[n] if s0 is None else s0 + p.ref[n], v, operand=s0)
    _check(case, variant, figs)
    assert not acc[v].any(), "the visible rows of acc come back zeroed"
    assert torch.equal(acc[~v], p.M32[~v]), "rows of culled Gaussians are not K8's to touch"


@CASES
def test_k8_overwrites_everything(lib_built, regime, flavour):
    """immediate flavour, accumulate = 0 into NaN-filled buffers: every element is overwritten, every visible row within its bar,
    culled rows exactly zero, d_means2D[:, 2] == 0"""
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    got, acc = d.k8(p.M32, d.outputs(nan_fill))
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), n
        assert not t[~p.visible].any(), n
    assert not got["means2D"][:, 2].any()
    _compare(p, got, acc, "immediate")


@pytest.mark.parametrize("regime", SIZE_CASES + SH_CASES)
def test_k8_unaligned_sh_rows(lib_built, regime):
    """dL/dshs one float off 16-byte alignment (sh_rows_out's scalar path), written and added into"""
    p, d = PR.prepared(regime), device_for(regime)
    got, acc = d.k8(p.M32, d.outputs(nan_fill, shs_offset=1))
    assert bool(torch.isfinite(got["shs"]).all()) and not got["shs"][~p.visible].any()
    _compare(p, got, acc, "immediate_unaligned")
    start = d.outputs(random_fill(p, 31), shs_offset=1)
    start_cpu = {n: t.cpu() for n, t in start.items()}
    got, acc = d.k8(p.M32, start, accumulate=ACC_ALL)
    _compare(p, got, acc, "accumulate_unaligned", start=start_cpu)
    assert torch.equal(got["shs"][~p.visible], start_cpu["shs"][~p.visible])


@pytest.mark.parametrize("mask", [ACC_ALL, 0b101010101])
@CASES
def test_k8_accumulate_masks(lib_built, regime, flavour, mask):
    """accumulate = TEXGS_ACC_ALL into random start values: start + gradient, culled rows bit-untouched.  The alternating mask
    0b101010101: the outputs whose bit is set are added into, the others overwritten -- a bit wired to the wrong output shows."""
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    start = d.outputs(random_fill(p, 17))
    start_cpu = {n: t.cpu() for n, t in start.items()}
    got, acc = d.k8(p.M32, start, accumulate=mask)
    added = {n: bool(mask & PR.ACC_BITS[n]) for n in got}
    _compare(p, got, acc, f"accumulate_{mask}", start={n: t for n, t in start_cpu.items() if added[n]})
    for n in got:
        if added[n]:
            assert torch.equal(got[n][~p.visible], start_cpu[n][~p.visible]), n
        else:
            assert not got[n][~p.visible].any(), n


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("regime,flavour", [(r, "textured") for r in ["general", "camera", "near_plane"] + SIZE_CASES + SH_CASES]
                         + [("general", "cov"), ("clamp", "coff")])
def test_k8_deferred_and_flush(lib_built, regime, flavour, unaligned):
    """DEFER (dL_dvd_residue set): K8 leaves dL/dshs alone and stores dL/dvd -- zero for culled rows and for degree 0 --; texgs_sh_flush
    then adds the SH rows and the view-direction term, and the sum is the same float64 total."""
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    case, v = p.case, p.visible
    fill = random_fill(p, 23)
    start = d.outputs(lambda n, shape: fill(n, shape) if n in ("shs", "means3D") else nan_fill(n, shape), shs_offset=int(unaligned))
    start_cpu = {n: t.cpu() for n, t in start.items()}
    residue = torch.full((case.N, 3), float("nan"), device=d.dev)
    got, acc = d.k8(p.M32, start, accumulate=PR.ACC_BITS["shs"] | PR.ACC_BITS["means3D"], residue=residue)
    res = residue.cpu()
    assert torch.equal(got["shs"], start_cpu["shs"]), "the DEFER flavour does not touch dL/dshs"
    assert bool(torch.isfinite(res).all()) and not res[~v].any()
    if case.sh_degree == 0:
        assert not res.any()
    else:
        A = PR.cotangent_from_moments(p.M32.to(PR.F64), p.pre, case.textured)[:, PR.R_VD:PR.R_VD + 3]
        assert torch.equal(res[v], A[v].to(torch.float32)), "the residue is dL/dvd, passed through"
    got = d.flush(start, residue)
    _compare(p, got, acc, "deferred" + ("_unaligned" if unaligned else ""), start={n: start_cpu[n] for n in ("shs", "means3D")})
    for n in ("shs", "means3D"):
        assert torch.equal(got[n][~v], start_cpu[n][~v]), n


@pytest.mark.parametrize("regime,flavour", [("general", "textured"), ("general", "cov"), ("size_257", "textured")])
def test_k8_without_want_gaussians_touches_nothing(lib_built, regime, flavour):
    p, d = PR.prepared(regime, flavour), device_for(regime, flavour)
    start = d.outputs(random_fill(p, 5))
    start_cpu = {n: t.cpu() for n, t in start.items()}
    got, acc = d.k8(p.M32, start, want=1)
    assert torch.equal(acc, p.M32)
    for n in got:
        assert torch.equal(got[n], start_cpu[n]), n


def test_k8_degenerate_plane_ignores_the_uv_cotangents(lib_built):
    """|sdot| <= 0.05 |t|: other values in the slots that become the g / G cotangents change no output of those rows, bit for bit (the
    float64 reference has G = g = 0 there, so the bars of test_k8_overwrites_everything already hold them to 'nothing flows')"""
    p, d = PR.prepared("degenerate_plane"), device_for("degenerate_plane")
    deg, reg = p.case.masks["degenerate"], p.case.masks["regular"]
    a, _ = d.k8(p.M32, d.outputs(nan_fill))
    b, _ = d.k8(PR.other_uv_cotangents(p.M32), d.outputs(nan_fill))
    for n in a:
        assert torch.equal(a[n][deg], b[n][deg]), n
    assert not torch.equal(a["means3D"][reg], b["means3D"][reg])
    assert not d.state["rec_shade"][deg][:, 0:8].any()
