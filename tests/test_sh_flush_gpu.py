"""-m gpu: the deferred SH gradient of a multi-view step (GradBucket.begin_deferred / flush_deferred, K8's DEFER flavour, texgs_sh_flush)
against the immediate accumulation of the same views: dL/dshs bit for bit, everything else as close as two immediate runs are to each
other (+ the one reassociated term per view in dL/dmeans3D); early flushes, clean state across steps and after an exception, the
pipeline's orders, and the entry point's refusals.  Small frames (128x96 at most), R = 64, K = 15."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
from texgs import synth

pytestmark = pytest.mark.gpu

W, H, R = 128, 96, 64
DEGREES = [3, 0, 1, 2, 3, 2, 1, 3, 0, 2]          # per view, mixed inside one step
NAMES = ["shs", "means3D", "opacities", "scales", "rotations", "uvs", "texture"]


def _cameras():
    """view 0 stands INSIDE the shell of Gaussians (radius ~1): about a third of them lie behind its near plane; the others look
    at the whole scene from outside"""
    return [synth.look_at_camera(np.array([0.3, 0.2, 0.4]), W, H)] + synth.fibonacci_cameras(9, W, H)


class Step:
    """One scene's leaves in a GradBucket whose shs slice starts at float offset 0 (16-byte aligned rows) or 1 (sh_rows_out's scalar path)."""

    def __init__(self, N, unaligned, seed=11):
        from texgs.multiview import GradBucket
        from texgs.rasterizer import GaussianRasterizationSettings
        self.dev = dev = torch.device("cuda:0")
        self.N = N
        scene = synth.make_scene(N, R, seed=seed, scale_mean=0.06)
        self.leaves = {n: getattr(scene, n).clone().to(dev).requires_grad_(True) for n in NAMES}
        self.m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
        self.juv = scene.gradient_uvs.to(dev)
        pad = [torch.zeros(1, device=dev, requires_grad=True)] if unaligned else []
        self.bucket = GradBucket(pad + [self.leaves[n] for n in NAMES] + [self.m2])
        off = dict(zip([id(p) for p in self.bucket.params], self.bucket.slices))
        self.slices = {n: off[id(self.leaves[n])] for n in NAMES}
        self.slices["means2D"] = off[id(self.m2)]
        assert self.slices["shs"][0] % 4 == (1 if unaligned else 0)
        self.cams = _cameras()
        self.sts = [Hh.settings_for(c, DEGREES[k], torch.zeros(3), device=dev, cls=GaussianRasterizationSettings)
                    for k, c in enumerate(self.cams)]
        target, nhat = synth.make_targets(H, W, seed=3)
        self.target, self.nhat = target.to(dev), nhat.to(dev)
        g = torch.Generator().manual_seed(5)
        self.start = (0.01 * torch.randn(self.bucket.flat.numel(), generator=g)).to(dev)      # the bucket does not start at zero

    def fwd(self, v):
        from texgs.rasterizer import GaussianRasterizer
        L = self.leaves
        out = GaussianRasterizer(self.sts[v], grad_sink=self.bucket)(
            means3D=L["means3D"], means2D=self.m2, shs=L["shs"], opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"],
            uvs=L["uvs"], gradient_uvs=self.juv, texture=L["texture"], extra_attrs=None)
        return synth.synthetic_loss(out[0], out[3], out[2], self.target, self.nhat)

    def reset(self, start=True):
        self.bucket.zero()
        if start:
            self.bucket.flat.copy_(self.start)

    def immediate(self, views, start=True):
        """the bucket used directly: nothing is deferred"""
        self.reset(start)
        for v in views:
            self.fwd(v).backward()
        torch.cuda.synchronize()
        return self.bucket.flat.clone()

    def deferred(self, views, start=True, depth=1, order="accumulate", pool=None):
        from texgs.multiview import ViewPipeline
        self.reset(start)
        if pool is not None:
            self.bucket.residue_pool_size = pool
        pipe = ViewPipeline(self.dev, depth=depth)
        try:
            pipe.run(views, self.fwd, lambda L: L.backward(), sink=self.bucket, order=order)
        finally:
            torch.cuda.synchronize()
            pipe.close()
        assert not self.bucket.deferred and not self.bucket._pending_sh
        return self.bucket.flat.clone()

    def part(self, flat, name):
        off, n = self.slices[name]
        return flat[off:off + n]


    def replayed(self, views, deferred, moments, record=False, pool=None):
        """The views in order on the current stream, immediate (the bucket used directly) or deferred (begin_deferred / flush_deferred),
        with K7's moment sums RECORDED into `moments` or PLAYED BACK from it: the bucket's before_accumulate hook runs between K7
        and K8, and the accumulator rows are this stream's cached scratch.  K7 adds its moments with fp32 atomics whose order
        changes from run to run; with them played back, two runs differ in nothing but K8 and the flush."""
        from texgs import rasterizer as RZ
        key = (self.dev.index, int(torch.cuda.current_stream(self.dev).cuda_stream))
        if key not in RZ._SCRATCH or RZ._SCRATCH[key].acc is None or RZ._SCRATCH[key].acc.shape[0] < self.N:
            self.immediate(views[:1])                                  # makes this stream's scratch
        acc = RZ._SCRATCH[key].acc
        it = iter(moments)
        self.reset()
        if pool is not None:
            self.bucket.residue_pool_size = pool
        if deferred:
            self.bucket.begin_deferred()
        self.bucket.before_accumulate = (lambda: moments.append(acc.clone())) if record else (lambda: acc.copy_(next(it)))
        try:
            for v in views:
                self.fwd(v).backward()
        finally:
            self.bucket.before_accumulate = None
            if deferred:
                self.bucket.flush_deferred()
        torch.cuda.synchronize()
        assert RZ._SCRATCH[key].acc is acc and len(moments) == len(views)
        return self.bucket.flat.clone()


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("nviews", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_deferred_equals_immediate(lib_built, N, nviews, unaligned):
    """The same views in the same order, immediate and deferred, into a bucket that starts non-zero.

    K7 sums its per-Gaussian moments with fp32 atomics, so two runs of ANY mode differ in the last bits and a difference between two
    single runs is a sample, not a bound (the first version of this test compared such samples and failed on a 1-ulp dL/dmeans2D at
    N = 1).  The moments of every view are therefore recorded in the first immediate run and played back into the second immediate
    run and into the deferred run (Step.replayed): the run-to-run figure of the immediate mode is then what K8 itself leaves open,
    and the deferred run is held to it.
    * dL/dshs: torch.equal.
    * every other per-Gaussian slice: at most the run-to-run figure of the two immediate runs (+ for dL/dmeans3D the reassociation of
      one term per view: the flush adds the view-direction term after the rest of the view's sum instead of inside it, at most one
      rounding of a partial sum per addition that moved -- bounded by 4 * views * 2^-24 * M, M = the largest |start| + sum over
      views of |that view's own dL/dmeans3D| (each view run alone), which is at least every partial sum of every element).
    * dL/dtexture is written by K7 and the bin reduce alone (atomics, not played back): relative L2 below 1e-5, the tolerance
      test_view_pipeline_streams_equal_serial gives a sum whose order changed.
    View 0 stands inside the shell; culled Gaussians get exactly nothing (the rows are compared bit for bit)."""
    st = Step(N, unaligned)
    views = list(range(nviews))
    tz = (torch.cat([st.leaves["means3D"].detach(), torch.ones(N, 1, device=st.dev)], 1) @ st.sts[0].viewmatrix)[:, 2]
    if N >= 255:
        assert 0.25 < float((tz <= 0.2).float().mean()) < 0.6, "view 0 should cull about a third of the Gaussians"
    moments = []
    imm = [st.replayed(views, False, moments, record=True), st.replayed(views, False, moments)]
    got = st.replayed(views, True, moments)
    assert st.bucket.sh_flushes == 1
    assert torch.equal(st.part(got, "shs"), st.part(imm[0], "shs")), \
        float((st.part(got, "shs") - st.part(imm[0], "shs")).abs().max())
    if N >= 255:
        assert float((st.part(got, "shs") - st.part(st.start, "shs")).abs().max()) > 0, "no SH gradient at all: the test sees nothing"
    alone = [st.part(st.immediate([v], start=False), "means3D").abs() for v in views]
    M = float((st.part(st.start, "means3D").abs() + sum(alone)).max())
    reassoc = 4 * nviews * 2.0 ** -24 * M
    for name in list(st.slices):
        if name == "shs":
            continue
        a, b, d = st.part(imm[0], name), st.part(imm[1], name), st.part(got, name)
        if name == "texture":
            rel = float((d.double() - a.double()).norm() / a.double().norm().clamp_min(1e-30))
            Hh.report(f"sh_flush/deferred_vs_immediate/N{N}_v{nviews}_{'un' if unaligned else ''}aligned/texture", rel_l2=rel)
            assert rel < 1e-5, rel
            continue
        run_to_run = float((a - b).abs().max())
        diff = float((d - a).abs().max())
        allowed = run_to_run + (reassoc if name == "means3D" else 0.0)
        Hh.report(f"sh_flush/deferred_vs_immediate/N{N}_v{nviews}_{'un' if unaligned else ''}aligned/{name}", deferred_diff=diff,
                  run_to_run=run_to_run, reassociation=reassoc if name == "means3D" else 0.0, grad_max=float(a.abs().max()))
        assert diff <= allowed, (name, diff, allowed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def test_early_flush_equals_one_flush(lib_built):
    """More views than the residue pool holds: the pool is flushed in the middle of the step (twice here), and the step equals the
    same step with a pool that holds them all.  On one stream with K7's moments played back (Step.replayed): the SH rows and every
    other per-Gaussian slice but dL/dmeans3D bit for bit (the order of the sums is the same), dL/dmeans3D within the reassociation
    bound of test_deferred_equals_immediate (an early flush adds the direction terms of its views before the later views' sums).  On
    three streams, where K7's atomics are not played back: rel L2 < 1e-5, and the pool has not grown."""
    st = Step(600, False)
    views = list(range(7))
    moments = []
    whole = st.replayed(views, True, moments, record=True)
    n0 = st.bucket.sh_flushes
    early = st.replayed(views, True, moments, pool=3)
    assert st.bucket.sh_flushes - n0 == 3            # 3 + 3 + 1 views
    for name in st.slices:
        if name not in ("means3D", "texture"):
            assert torch.equal(st.part(early, name), st.part(whole, name)), name
    alone = [st.part(st.immediate([v], start=False), "means3D").abs() for v in views]
    M = float((st.part(st.start, "means3D").abs() + sum(alone)).max())
    diff = float((st.part(early, "means3D") - st.part(whole, "means3D")).abs().max())
    Hh.report("sh_flush/early_flush_vs_one/means3D", diff=diff, reassociation=4 * len(views) * 2.0 ** -24 * M)
    assert diff <= 4 * len(views) * 2.0 ** -24 * M
    st = Step(600, False)                            # the same scene in a bucket of its own, whose pool starts empty
    piped = st.deferred(views, pool=3, depth=3)
    assert st.bucket.sh_flushes == 3
    rel = _rel(piped, whole)
    Hh.report("sh_flush/early_flush_3_streams_vs_one", rel_l2=rel, rel_l2_shs=_rel(st.part(piped, "shs"), st.part(whole, "shs")))
    assert rel < 1e-5 and _rel(st.part(piped, "shs"), st.part(whole, "shs")) < 1e-5
    assert [len(p) for p in st.bucket._residues.values()] == [3]


def test_clean_state_across_steps_and_after_an_exception(lib_built):
    """Two steps back to back with a zero() in between (a third, of other views, between them, so that other residues sit in the pool's
    buffers): with K7's moments played back the second equals the first bit for bit in every per-Gaussian slice -- no residue of one
    step in the next --, and nothing is pending after a step.  An exception inside backward_fn: `finally` still flushes the views
    that ran and leaves the mode (their SH rows against the immediate sum of the same views: rel L2 < 1e-5, K7 not played back)."""
    from texgs.multiview import ViewPipeline
    st = Step(500, False)
    views = [0, 1, 2, 3]
    moments = []
    first = st.replayed(views, True, moments, record=True)
    other = st.deferred([4, 5, 6], start=False)
    again = st.replayed(views, True, moments)
    assert other.shape == first.shape and not st.bucket.deferred and not st.bucket._pending_sh and not st.bucket._residues_used
    for name in st.slices:
        if name != "texture":
            assert torch.equal(st.part(first, name), st.part(again, name)), name
    ref2 = st.immediate(views[:2], start=False)
    st.reset(start=False)
    count = [0]

    def bwd(L):
        count[0] += 1
        if count[0] == 3:
            raise RuntimeError("boom")
        L.backward()
    pipe = ViewPipeline(st.dev, depth=2)
    with pytest.raises(RuntimeError, match="boom"):
        pipe.run(views, st.fwd, bwd, sink=st.bucket, order="accumulate")
    torch.cuda.synchronize()
    pipe.close()
    assert not st.bucket.deferred and not st.bucket._pending_sh and not st.bucket._residues_used
    rel = _rel(st.part(st.bucket.flat, "shs"), st.part(ref2, "shs"))
    Hh.report("sh_flush/after_exception/shs_vs_immediate", rel_l2=rel)
    assert rel < 1e-5, rel                                                       # the two views that ran were flushed
    st.bucket.zero()                                                             # (asserts that nothing is pending)


@pytest.mark.parametrize("depth,order", [(1, "accumulate"), (1, "none"), (3, "accumulate"), (3, "none")])
def test_pipeline_orders_equal_serial(lib_built, depth, order):
    """ViewPipeline at depth 1 and 3, orders "accumulate" and "none", deferred, against the serial immediate accumulation: the
    tolerance of test_view_pipeline_streams_equal_serial (rel L2 < 1e-5); two steps, so the replicas and the pool come back clean."""
    st = Step(1000, False)
    views = list(range(7))
    whole = st.immediate(views, start=False).double()
    for _ in range(2):
        got = st.deferred(views, start=False, depth=depth, order=order).double()
    rel = float((whole - got).norm() / whole.norm())
    rel_shs = float((st.part(whole, "shs") - st.part(got, "shs")).norm() / st.part(whole, "shs").norm())
    Hh.report(f"sh_flush/pipeline_depth{depth}_{order}_vs_serial", rel_l2=rel, rel_l2_shs=rel_shs, max_abs=float((whole - got).abs().max()))
    assert rel < 1e-5 and rel_shs < 1e-5, (rel, rel_shs)
    assert st.bucket.active == 0 and st.bucket.before_accumulate is None


def test_outside_the_pipeline_nothing_is_deferred(lib_built):
    """A bucket used directly (plain loop over views) never enters the mode: no residue buffer is made, no flush is launched."""
    st = Step(300, False)
    st.immediate([0, 1])
    assert st.bucket.sh_flushes == 0 and not st.bucket._residues and not st.bucket.deferred


def test_entry_point_refusals(lib_built):
    """texgs_sh_flush refuses, by name and before any launch: a view count above the maximum, a NULL sink with views pending, a K that
    does not match the one a view's residue was written with; a degree outside 0..3; K8 refuses a residue without both accumulate bits."""
    from texgs import _lib
    from texgs.multiview import SH_FLUSH_MAX_VIEWS, ShFlushView, sh_flush_entry
    fn, lib = sh_flush_entry(), _lib.load()
    dev = torch.device("cuda:0")
    N, K = 10, 15
    m3, shs = torch.zeros(N, 3, device=dev), torch.zeros(N, K, 3, device=dev)
    d_shs, d_m3 = torch.ones(N, K, 3, device=dev), torch.ones(N, 3, device=dev)
    cp, res = torch.zeros(3, device=dev), torch.ones(N, 3, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def recs(n, k=K, deg=3):
        return (ShFlushView * n)(*[ShFlushView(cp.data_ptr(), res.data_ptr(), deg, k) for _ in range(n)])

    def refused(text, *args):
        assert fn(*args) != 0
        assert text in lib.texgs_last_error().decode(), lib.texgs_last_error()
    p = lambda t: t.data_ptr()
    refused("TEXGS_SH_FLUSH_MAX_VIEWS", N, K, p(m3), p(shs), p(d_shs), p(d_m3), recs(SH_FLUSH_MAX_VIEWS + 1), SH_FLUSH_MAX_VIEWS + 1, stream)
    refused("NULL sink", N, K, p(m3), p(shs), None, p(d_m3), recs(2), 2, stream)
    refused("NULL sink", N, K, p(m3), p(shs), p(d_shs), None, recs(2), 2, stream)
    refused("K does not match", N, K, p(m3), p(shs), p(d_shs), p(d_m3), recs(2, k=K - 1), 2, stream)
    refused("sh_degree", N, K, p(m3), p(shs), p(d_shs), p(d_m3), recs(1, deg=4), 1, stream)
    refused("count < 0", N, K, p(m3), p(shs), p(d_shs), p(d_m3), recs(1), -1, stream)
    assert fn(N, K, p(m3), p(shs), None, None, None, 0, stream) == 0          # nothing pending: a no-op, whatever the pointers
    torch.cuda.synchronize()
    assert float(d_shs.min()) == 1.0 and float(d_m3.min()) == 1.0             # a refused call has changed nothing
    with pytest.raises(RuntimeError, match="texgs_sh_flush failed"):
        _lib.call(fn, N, K, p(m3), p(shs), None, p(d_m3), recs(1), 1, stream)
    # zero shs and a unit residue: the rows get exactly b_k(dir) * 1, the means nothing (dd = 0)
    m3[:, 2] = 2.0
    assert fn(N, K, p(m3), p(shs), p(d_shs), p(d_m3), recs(1), 1, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_m3, torch.ones_like(d_m3))
    c1 = np.float32(0.4886025119029199)
    assert torch.equal(d_shs[:, 1, :].cpu(), torch.full((N, 3), float(np.float32(1.0) + c1 * np.float32(1.0))))      # b_1 = C1 * z, dir = (0,0,1)
    grads = _lib.Grads()
    grads.want, grads.acc, grads.dL_dvd_residue, grads.accumulate = _lib.WANT_GAUSSIANS, p(res), p(res), 1
    frame = _lib.Frame(H, W, 0.3, 0.3, 1.0, 3, K, R, N, 0, p(cp), p(cp), p(cp), p(cp))
    inputs, geom = _lib.Inputs(), _lib.Geom()
    assert lib.texgs_backward_preprocess(C.byref(frame), C.byref(inputs), C.byref(geom), C.byref(grads), stream) != 0
    assert b"dL_dvd_residue" in lib.texgs_last_error()
