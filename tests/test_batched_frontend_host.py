"""-m "not gpu": the host side of the batched front end -- the new entry points' signatures against include/texgs_multiview.h, what
they refuse before any launch, the grouping rule of texgs.rasterizer.batched_prefetch, the step buffers' accounting, and
ViewPipeline.run's use of the batch scope (with recorded streams; no device)."""
import ctypes
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_signatures_match_the_header(lib_built):
    """views_signatures() against the prototypes of include/texgs_multiview.h: names, argument counts, struct pointers and scalars; the
    library exports every one; the ABI number is unchanged (the addition is additive: no struct or earlier entry point moved)"""
    from texgs import _lib
    from texgs import multiview as MV
    hdr = os.path.join(INC, "texgs_multiview.h")
    sigs = MV.views_signatures()
    assert sigs is MV.views_signatures()            # a table built once
    assert set(abi_check.prototypes(hdr)) == set(sigs) | {"texgs_sh_flush"}
    mirror = {"TexGSFrame": _lib.Frame, "TexGSInputs": _lib.Inputs, "TexGSGeom": _lib.Geom, "TexGSBinning": _lib.Binning, "TexGSImage": _lib.Image,
              "TexGSShFlushView": MV.ShFlushView}
    assert abi_check.signature_mismatches(hdr, {"texgs_sh_flush": MV.SH_FLUSH_SIGNATURE, **sigs}, mirror) == []
    lib = ctypes.CDLL(lib_built)
    assert all(restype is ctypes.c_int and hasattr(lib, name) for name, (restype, _) in sigs.items())
    hdr = open(hdr).read()
    assert int(re.search(r"#define\s+TEXGS_BATCH_MAX_VIEWS\s+(\d+)", hdr).group(1)) == MV.BATCH_MAX_VIEWS == 16
    assert _lib.load().texgs_abi_version() == _lib.ABI_VERSION


def test_entry_points_refuse_by_name_before_any_launch(lib_built):
    """More than 16 views, mixed image sizes, mixed sh_degree, N == 0, a short scan_temp: each is refused with its reason and nothing is
    launched (no device is needed to find that out) -- the host layer then takes the per-view path"""
    from texgs import _lib
    from texgs import multiview as MV
    lib, ent = _lib.load(), MV.views_entries()

    def frames(n, **over):
        fs = [_lib.Frame(64, 64, 0.3, 0.3, 1.0, 3, 15, 4, 100, 0, 1, 1, 1, 1) for _ in range(n)]
        for k, v in over.items():
            setattr(fs[-1], k, v)
        return (_lib.Frame * n)(*fs)
    inputs = _lib.Inputs(1, 1, 1, 1, 1, 1, 1, 1, None, None)
    geoms = (_lib.Geom * 17)(*[_lib.Geom(1, 1, 1, 1, 1, 1, 1, 1, 16) for _ in range(17)])

    def refused(rc, text):
        assert rc != 0 and text in lib.texgs_last_error(), lib.texgs_last_error()
    refused(ent.preprocess_forward_views(frames(17), ctypes.byref(inputs), geoms, 17, 1, None), b"TEXGS_BATCH_MAX_VIEWS")
    refused(ent.preprocess_forward_views(frames(2), ctypes.byref(inputs), geoms, 0, 1, None), b"count < 1")
    refused(ent.preprocess_forward_views(frames(2, image_width=80), ctypes.byref(inputs), geoms, 2, 1, None), b"one image size")
    refused(ent.preprocess_forward_views(frames(2, sh_degree=2), ctypes.byref(inputs), geoms, 2, 1, None), b"one sh_degree")
    refused(ent.preprocess_forward_views(frames(2, num_gaussians=99), ctypes.byref(inputs), geoms, 2, 1, None), b"one num_gaussians")
    refused(ent.preprocess_forward_views(frames(2), ctypes.byref(inputs), geoms, 2, 1, None), b"scan_temp too small")
    zero = frames(2)
    zero[0].num_gaussians = zero[1].num_gaussians = 0
    refused(ent.preprocess_forward_views(zero, ctypes.byref(inputs), geoms, 2, 1, None), b"per-view path")
    refused(ent.depth_sort_scan_views(geoms, 100, 17, None), b"TEXGS_BATCH_MAX_VIEWS")
    refused(ent.depth_sort_scan_views(geoms, 100, 2, None), b"scan_temp too small")
    bins = (_lib.Binning * 2)(*[_lib.Binning(5, 1, 1, 1, 1, 1, 1, 8) for _ in range(2)])
    imgs = (_lib.Image * 2)()
    refused(ent.bin_sort_views(frames(2), geoms, bins, imgs, 2, None), b"sort_temp too small")
    refused(ent.bin_sort_views(frames(2, image_height=96), geoms, bins, imgs, 2, None), b"one image size")


def test_grouping_rule():
    """Equal keys go together in first-seen order; a group needs two views; more than max_views are cut into runs; what is left alone
    takes the per-view path.  The number of tiles never splits a group: the views are a grid dimension of the tile sort, so there is no
    V * T limit to decide on."""
    from texgs.rasterizer import group_requests
    assert group_requests([], 16) == ([], [])
    assert group_requests(["a"], 16) == ([], [0])
    assert group_requests(["a", "a", "a"], 16) == ([[0, 1, 2]], [])
    # mixed sizes and mixed tensors: the key differs, the groups split; the single one is left alone
    assert group_requests([("t1", 256), ("t1", 200), ("t1", 256), ("t2", 256), ("t1", 200)], 16) == ([[0, 2], [1, 4]], [3])
    # V > 16: runs of 16; a run of one falls back
    groups, rest = group_requests(["a"] * 17, 16)
    assert groups == [list(range(16))] and rest == [16]
    groups, rest = group_requests(["a"] * 35 + ["b"], 16)
    assert [len(g) for g in groups] == [16, 16, 3] and rest == [35]
    # min_views = 1 (tests of the entry points with count = 1): nothing is left alone
    assert group_requests(["a", "b", "a"], 16, min_views=1) == ([[0, 2], [1]], [])


def test_parked_batched_forwards_are_dropped_when_the_next_scope_batches():
    """A batched forward that no view picked up keeps its group's step buffers alive: _drop_parked_batched (called when a later scope
    batches) removes those and only those from the table of begun forwards"""
    from types import SimpleNamespace
    from texgs import rasterizer as RZ
    saved = dict(RZ._PREFETCH)
    try:
        RZ._PREFETCH.clear()
        per_view, stale = SimpleNamespace(binned=None), SimpleNamespace(binned=(7, 1, None))
        RZ._PREFETCH[(0, 11)] = [("k1", stale), ("k2", per_view)]
        RZ._PREFETCH[(0, 12)] = [("k3", stale)]
        RZ._drop_parked_batched()
        assert RZ._PREFETCH == {(0, 11): [("k2", per_view)]}
    finally:
        RZ._PREFETCH.clear()
        RZ._PREFETCH.update(saved)


def test_batch_key_tells_inputs_sizes_and_degree_apart():
    from texgs import rasterizer as RZ
    m = torch.zeros(4, 3)
    st = lambda **kw: RZ.GaussianRasterizationSettings(**{**dict(image_height=64, image_width=64, tanfovx=0.3, tanfovy=0.3, bg=torch.zeros(3),
                                                                scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=3,
                                                                campos=torch.zeros(3), prefiltered=False, debug=False), **kw})
    fwd = lambda s, t: RZ._Forward(s, (t, None, None, None, None, None, None, None, None, None), True, None, False)
    k0 = RZ._batch_key(fwd(st(), m))
    assert k0 == RZ._batch_key(fwd(st(viewmatrix=torch.ones(4, 4), campos=torch.ones(3), tanfovx=0.5), m))      # another camera: same group
    assert k0 != RZ._batch_key(fwd(st(image_width=80), m))
    assert k0 != RZ._batch_key(fwd(st(sh_degree=2), m))
    assert k0 != RZ._batch_key(fwd(st(), m.clone()))
    m.add_(1.0)                                                                                                # a new version of the same storage
    assert k0 != RZ._batch_key(fwd(st(), m))


def test_step_buffer_accounting_returns_to_zero():
    """Arenas placed in a step buffer keep it alive and are counted in scratch_bytes(); when the last one goes, so does the buffer"""
    from texgs import rasterizer as RZ
    base = RZ.scratch_bytes()
    dev = torch.device("cpu")
    a, b = RZ._Arena(dev), RZ._Arena(dev)
    a.add("x", (10,), torch.int32)
    a.add("y", (3, 5), torch.float32)
    b.add("x", (7,), torch.int64)
    sb = RZ._StepBuffer(1024 + 256, dev)
    a.place(sb, 0)
    b.place(sb, 512)
    assert RZ.step_buffer_bytes() == 1280 and RZ.scratch_bytes() == base + 1280
    a.view("y").fill_(2.0)
    b.view("x").fill_(-1)
    assert a.ptr("y") == sb.buf.data_ptr() + 256 and b.ptr("x") == sb.buf.data_ptr() + 512
    assert float(a.view("y").sum()) == 30.0 and int(b.view("x").sum()) == -7          # the pieces do not overlap
    del sb, a
    assert RZ.step_buffer_bytes() == 1280                                             # b still holds it
    del b
    RZ.release_scratch()
    assert RZ.step_buffer_bytes() == 0 and RZ.scratch_bytes() == base


def test_view_pipeline_registers_every_view_inside_one_scope(monkeypatch):
    """On a GPU pipeline ViewPipeline.run calls prefetch_fn for EVERY view before the loop, each under the stream the view will run on,
    inside ONE batched_prefetch scope; views the scope batched are not prefetched again, views it left alone keep the one-view-per-
    stream-ahead rhythm; batch=False and a pipeline that is not on a GPU keep today's calls exactly."""
    import contextlib
    import texgs.multiview as MV
    from texgs import rasterizer as RZ
    log = []

    class FakeEvent:
        def record(self, stream):
            pass

    class FakeStream:
        def __init__(self, name):
            self.name = name

        def wait_stream(self, other):
            pass

        def wait_event(self, ev):
            pass
    current = [FakeStream("main")]

    @contextlib.contextmanager
    def fake_stream_ctx(s):
        current.append(s)
        try:
            yield
        finally:
            current.pop()
    monkeypatch.setattr(MV.torch.cuda, "Event", FakeEvent)
    monkeypatch.setattr(MV.torch.cuda, "stream", fake_stream_ctx)
    monkeypatch.setattr(MV.torch.cuda, "current_stream", lambda dev=None: current[-1])
    leave_alone = set()

    class FakeScope:
        def __init__(self, begin_rest=True):
            assert begin_rest is False
            self.requests = []

        def __enter__(self):
            log.append(("scope", "enter"))
            RZ._BATCH_SCOPE = self
            return self

        def __exit__(self, *exc):
            RZ._BATCH_SCOPE = None
            for r in self.requests:
                r.batched = r.fwd not in leave_alone
            log.append(("scope", "exit", current[-1].name))
            return False
    monkeypatch.setattr(RZ, "batched_prefetch", FakeScope)

    def pre(v):
        if RZ._BATCH_SCOPE is not None:
            RZ._BATCH_SCOPE.requests.append(RZ._Request(v, current[-1]))
            log.append(("register", current[-1].name, v))
        else:
            log.append(("begin", current[-1].name, v))

    def run(depth, nviews, device="cuda", **kw):
        log.clear()
        p = MV.ViewPipeline.__new__(MV.ViewPipeline)
        p.device = torch.device(device)
        p.streams = [FakeStream(f"s{k}") for k in range(depth)] if depth > 1 else []
        p.run(list(range(nviews)), lambda v: log.append(("fwd", current[-1].name, v)) or v, lambda v: log.append(("bwd", current[-1].name, v)),
              sink=None, order="backward", prefetch_fn=pre, **kw)
        return list(log)
    lg = run(3, 5)
    assert lg[:8] == [("scope", "enter")] + [("register", f"s{v % 3}", v) for v in range(5)] + [("scope", "exit", "main"), ("fwd", "s0", 0)]
    assert not [e for e in lg if e[0] == "begin"]
    leave_alone.update({1, 4})
    lg = run(3, 5)
    assert [e for e in lg if e[0] == "begin"] == [("begin", "s1", 1), ("begin", "s1", 4)]
    assert lg.index(("begin", "s1", 1)) < lg.index(("fwd", "s0", 0)) and lg[lg.index(("fwd", "s1", 1)) + 1] == ("begin", "s1", 4)
    leave_alone.clear()
    lg = run(1, 3)
    assert lg[:5] == [("scope", "enter"), ("register", "main", 0), ("register", "main", 1), ("register", "main", 2), ("scope", "exit", "main")]
    assert [e[0] for e in lg[5:]] == ["fwd", "bwd"] * 3
    for kw in (dict(batch=False), dict(device="cpu")):
        lg = run(3, 5, **kw)
        assert not [e for e in lg if e[0] in ("scope", "register")]
        assert lg[:3] == [("begin", "s0", 0), ("begin", "s1", 1), ("begin", "s2", 2)] and lg[lg.index(("fwd", "s0", 0)) + 1] == ("begin", "s0", 3)
