"""No GPU: the bookkeeping of GradBucket's deferred SH gradient (mode on / off, pool reuse, what zero / all_reduce / wait insist on),
the record struct's layout against include/texgs_multiview.h, and ViewPipeline with a sink that lacks the new methods."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _bucket(N=6, K=15):
    from texgs.multiview import GradBucket
    m3 = torch.zeros(N, 3, requires_grad=True)
    shs = torch.zeros(N, K, 3, requires_grad=True)
    op = torch.zeros(N, 1, requires_grad=True)
    return GradBucket([m3, shs, op]), m3, shs, op


def test_mode_pool_and_asserts(monkeypatch):
    import texgs.multiview as MV
    bucket, m3, shs, op = _bucket()
    cp = torch.zeros(3)
    # off by default; a bucket used directly never defers
    assert not bucket.deferred and not bucket.wants_deferred(m3, shs)
    bucket.begin_deferred()
    assert bucket.deferred and bucket.wants_deferred(m3, shs)
    # both tensors must be sunk into the bucket
    other = torch.zeros(6, 15, 3, requires_grad=True)
    assert not bucket.wants_deferred(m3, other) and not bucket.wants_deferred(other, shs) and not bucket.wants_deferred(m3, None)
    assert not bucket.wants_deferred(m3, m3)
    r0 = bucket.sh_residue_for(m3, shs, m3, shs, cp, 3)
    r1 = bucket.sh_residue_for(m3, shs, m3, shs, cp, 1)
    assert r0.shape == (6, 3) and r0.dtype == torch.float32 and r0.data_ptr() != r1.data_ptr()
    assert [e[5] for e in bucket._pending_sh] == [3, 1] and bucket._pending_sh[0][6] is r0
    # with views pending, nothing may read or clear the bucket
    for call in (bucket.zero, bucket.wait, lambda: bucket.all_reduce(None), lambda: bucket.all_reduce_async(None),
                 bucket.begin_deferred):
        with pytest.raises(AssertionError, match="pending"):
            call()
    # ... except a segment that the flush does not add into (the texture half, all-reduced from inside the last view's backward)
    with pytest.raises(AssertionError, match="pending"):
        bucket.all_reduce_async(None, bucket.segment_of([shs]))
    with pytest.raises(AttributeError):             # past the check: it goes on to ask the (absent) process group for its backend
        bucket.all_reduce_async(None, bucket.segment_of([op]))
    # the flush: one call per run of at most SH_FLUSH_MAX_VIEWS views, in registration order, into the slices of `flat`
    calls = []

    def fake_call(fn, N, K, p_m3, p_shs, p_dshs, p_dm3, recs, count, stream):
        calls.append((N, K, p_m3, p_shs, p_dshs, p_dm3, [(recs[k].residue, recs[k].sh_degree, recs[k].sh_coeffs) for k in range(count)]))

    import contextlib
    from texgs import _lib
    monkeypatch.setattr(MV, "sh_flush_entry", lambda: "fn")
    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(_lib, "on", lambda device: contextlib.nullcontext(0))
    bucket.flush_deferred()
    assert not bucket.deferred and not bucket._pending_sh and bucket.sh_flushes == 1
    off_m3, off_shs = bucket.slices[0][0], bucket.slices[1][0]
    assert calls == [(6, 15, m3.data_ptr(), shs.data_ptr(), bucket.flat.data_ptr() + 4 * off_shs, bucket.flat.data_ptr() + 4 * off_m3,
                      [(r0.data_ptr(), 3, 15), (r1.data_ptr(), 1, 15)])]
    bucket.zero()
    bucket.wait()
    # the pool is reused by the next step, in order; it grows only while views are pending
    bucket.begin_deferred()
    assert bucket.sh_residue_for(m3, shs, m3, shs, cp, 2) is r0 and bucket.sh_residue_for(m3, shs, m3, shs, cp, 2) is r1
    assert len(bucket._residues[(6, m3.device)]) == 2
    # a full pool asks for an early flush; without early flushes (order="none") it grows instead
    bucket.residue_pool_size = 2
    assert bucket.deferred_pool_full(m3)
    bucket.flush_pending()
    assert bucket.deferred and not bucket.deferred_pool_full(m3) and bucket.sh_flushes == 2
    assert bucket.sh_residue_for(m3, shs, m3, shs, cp, 2) is r0
    bucket.flush_deferred()
    bucket.begin_deferred(early_flush=False)
    for _ in range(3):
        bucket.sh_residue_for(m3, shs, m3, shs, cp, 2)
    assert not bucket.deferred_pool_full(m3) and len(bucket._residues[(6, m3.device)]) == 3
    # more views than one launch carries: several launches, the order kept
    for _ in range(MV.SH_FLUSH_MAX_VIEWS):
        bucket.sh_residue_for(m3, shs, m3, shs, cp, 1)
    calls.clear()
    bucket.flush_deferred()
    assert [len(c[6]) for c in calls] == [MV.SH_FLUSH_MAX_VIEWS, 3] and [d for c in calls for _, d, _ in c[6]] == [2] * 3 + [1] * 16
    # a flush with nothing pending launches nothing
    calls.clear()
    bucket.begin_deferred()
    bucket.flush_deferred()
    assert calls == [] and not bucket.deferred


def test_pipeline_brackets_the_step_and_leaves_other_sinks_alone():
    """ViewPipeline.run at depth 1: begin_deferred before the first view, flush_deferred after the last -- also when a view raises --
    and only with a backward; a sink without the two methods is driven exactly as before."""
    from texgs.multiview import ViewPipeline
    log = []

    class Sink:
        before_accumulate = None

        def begin_deferred(self, early_flush=True):
            log.append(("begin", early_flush))

        def flush_deferred(self):
            log.append("flush")
    pipe = ViewPipeline("cpu", depth=1)
    res = pipe.run([1, 2], lambda v: log.append(("f", v)) or v, lambda o: log.append(("b", o)), sink=Sink())
    assert res == [1, 2] and log == [("begin", True), ("f", 1), ("b", 1), ("f", 2), ("b", 2), "flush"]
    log.clear()
    with pytest.raises(RuntimeError):
        pipe.run([1, 2], lambda v: v, lambda o: (_ for _ in ()).throw(RuntimeError("boom")), sink=Sink())
    assert log == [("begin", True), "flush"]
    log.clear()
    pipe.run([1], lambda v: log.append(("f", v)) or v, None, sink=Sink())        # forward only: nothing to defer
    assert log == [("f", 1)]

    class Old:                                  # the part of a sink the pipeline used before
        before_accumulate = None
    log.clear()
    assert pipe.run([3], lambda v: log.append(("f", v)) or v, lambda o: log.append(("b", o)), sink=Old()) == [3]
    assert log == [("f", 3), ("b", 3)]

    class Half(Old):                            # begin without flush: not a deferring sink
        def begin_deferred(self, early_flush=True):
            log.append("begin")
    log.clear()
    pipe.run([3], lambda v: v, lambda o: None, sink=Half())
    assert log == []


def test_record_struct_matches_the_header(tmp_path):
    """ShFlushView (texgs/multiview.py) against TexGSShFlushView: size, offsets, the maximum; the header is plain C99 and declares
    texgs_sh_flush with the argument list of SH_FLUSH_SIGNATURE; the library exports it (cross-compiled: no GPU needed)."""
    from texgs import _lib
    from texgs import multiview as MV
    mirrors = {"TexGSShFlushView": MV.ShFlushView}
    assert abi_check.layout_mismatches("texgs_multiview.h", mirrors, {"TEXGS_SH_FLUSH_MAX_VIEWS": MV.SH_FLUSH_MAX_VIEWS}, tmp_path) == []
    assert ctypes.sizeof(MV.ShFlushView) == 24 and MV.SH_FLUSH_MAX_VIEWS == 16
    hdr = os.path.join(INC, "texgs_multiview.h")
    assert len(abi_check.prototypes(hdr)["texgs_sh_flush"][1]) == len(MV.SH_FLUSH_SIGNATURE[1]) == 9
    table = {"texgs_sh_flush": MV.SH_FLUSH_SIGNATURE, **MV.views_signatures()}       # the header's other entry points: the batched front end's
    texgs_h = {"TexGSFrame": _lib.Frame, "TexGSInputs": _lib.Inputs, "TexGSGeom": _lib.Geom, "TexGSBinning": _lib.Binning, "TexGSImage": _lib.Image}
    assert abi_check.signature_mismatches(hdr, table, {**texgs_h, **mirrors}) == []
    assert hasattr(_lib.load(), "texgs_sh_flush")
    # the new TexGSGrads field is the struct's last: a zero-filled struct of the old size means "not deferred"
    assert _lib.Grads._fields_[-1][0] == "dL_dvd_residue" and _lib.Grads._fields_[-2][0] == "accumulate"
