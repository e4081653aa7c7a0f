"""Multi-view (frame-sharded) training path: one process per GPU, views sharded over ranks, parameters
replicated, ONE collective per step -- an all-reduce (SUM) of a single flat fp32 gradient bucket over RCCL/xGMI
(SURVEY.md section 8e).  The reference has no distributed code (train.py:138-149 is one view per step on one
GPU); this is the data-parallel layer the north star adds around the operator, nothing more.

xGMI is point-to-point (7 links x ~153 GB/s per GPU): a ~143 MB bucket all-reduced once per 8-view step costs
O(1-2 ms) against O(10 ms) of rendering.  The bucket is flat so RCCL sees large messages, and it is reduced as TWO
segments on a side stream (GradBucket.all_reduce_async): the texture gradient (half the bytes) as soon as the last
view's texture-gradient reduce kernel has been issued -- it then overlaps the remaining K8 launches and the host's
end-of-step work --, the per-Gaussian gradients after the last K8; the compute stream waits for both only before the
gradients are read (GradBucket.wait).  Views are dealt to ranks by estimated cost (lpt_shard_views), not round-robin:
the step ends with the slowest rank.
"""
import contextlib
import ctypes as C
from typing import List, Sequence

import torch

from . import _lib

SH_FLUSH_MAX_VIEWS = 16         # TEXGS_SH_FLUSH_MAX_VIEWS: view records of one texgs_sh_flush launch


class ShFlushView(C.Structure):
    """ctypes mirror of TexGSShFlushView (include/texgs_multiview.h), 24 bytes"""
    _fields_ = [("campos", C.c_void_p), ("residue", C.c_void_p), ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32)]


# (restype, argtypes) of `int texgs_sh_flush(int32_t N, int32_t K, const float* means3D, const float* shs, float* dL_dshs,
#  float* dL_dmeans3D, const TexGSShFlushView* views, int32_t count, void* stream)`
SH_FLUSH_SIGNATURE = (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ShFlushView), C.c_int32,
                                C.c_void_p])
_SH_FLUSH_SIGNATURES = {"texgs_sh_flush": SH_FLUSH_SIGNATURE}


def sh_flush_entry():
    """texgs_sh_flush of the loaded library with its signature applied (on first use)"""
    return _lib.bind(_SH_FLUSH_SIGNATURES).texgs_sh_flush


BATCH_MAX_VIEWS = 16            # TEXGS_BATCH_MAX_VIEWS: views of one batched front end (K1..K5 once per step, texgs.rasterizer.batched_prefetch)
_P = C.POINTER
_VIEWS_SIGNATURES = {
    "texgs_preprocess_forward_views": (C.c_int, [_P(_lib.Frame), _P(_lib.Inputs), _P(_lib.Geom), C.c_int32, C.c_void_p, C.c_void_p]),
    "texgs_depth_sort_scan_views": (C.c_int, [_P(_lib.Geom), C.c_int32, C.c_int32, C.c_void_p]),
    "texgs_bin_sort_views": (C.c_int, [_P(_lib.Frame), _P(_lib.Geom), _P(_lib.Binning), _P(_lib.Image), C.c_int32, C.c_void_p]),
    "texgs_render_forward_binned": (C.c_int, [_P(_lib.Frame), _P(_lib.Inputs), _P(_lib.Geom), _P(_lib.Binning), _P(_lib.Image), C.c_void_p]),
}
_views_fns = None


def views_signatures():
    """name -> (restype, argtypes) of the batched front end's entry points (include/texgs_multiview.h), in the header's order; the structs
    are texgs.h's, passed as arrays of `count` elements"""
    return _VIEWS_SIGNATURES


def views_entries():
    """The batched front end's entry points of the loaded library with their signatures applied (on first use), by name without `texgs_`"""
    global _views_fns
    if _views_fns is None:
        from types import SimpleNamespace
        lib = _lib.bind(_VIEWS_SIGNATURES)
        _views_fns = SimpleNamespace(**{name[len("texgs_"):]: getattr(lib, name) for name in _VIEWS_SIGNATURES})
    return _views_fns


def shard_views(num_views: int, rank: int, world: int) -> List[int]:
    """Round-robin frame sharding: rank r renders views r, r+world, ...  Every view belongs to exactly one rank."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    views = list(range(rank, num_views, world))
    if not views:
        raise ValueError(f"rank {rank} gets no view: {num_views} views over {world} ranks")
    return views


def lpt_shard_views(costs: Sequence[float], rank: int, world: int) -> List[int]:
    """Longest-processing-time-first sharding: views sorted by estimated cost (e.g. the instance count D of the view's last
    render: K6 / K7 time is proportional to it) are dealt, most expensive first, to the rank with the smallest load so far.
    Deterministic (ties by view index), every view belongs to exactly one rank, every rank gets the same NUMBER of views
    when num_views is a multiple of world (the ranks of a step must issue the same number of collectives and the driver's
    bench counts views)."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    n = len(costs)
    if n < world:
        raise ValueError(f"{n} views over {world} ranks")
    order = sorted(range(n), key=lambda v: (-float(costs[v]), v))
    quota = [n // world + (1 if r < n % world else 0) for r in range(world)]
    load = [0.0] * world
    mine = [[] for _ in range(world)]
    for v in order:
        r = min((r for r in range(world) if len(mine[r]) < quota[r]), key=lambda r: (load[r], r))
        mine[r].append(v)
        load[r] += float(costs[v])
    return sorted(mine[rank])


class GradBucket:
    """One flat fp32 buffer that backs the .grad of every parameter, so that (a) autograd accumulates the views
    of a step in place, and (b) the whole gradient is all-reduced with a single collective."""

    def __init__(self, params: Sequence[torch.Tensor]):
        self.params = [p for p in params if p is not None and p.requires_grad]
        if not self.params:
            raise ValueError("no parameter requires grad")
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        self.slices = []
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("GradBucket needs float32 parameters on one device")
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            self.slices.append((off, n))
            off += n
        # ViewPipeline state: replica buffers (one per extra stream) that kernels accumulate into instead of `flat`, the
        # replica in use, and the hook the rasterizer's backward calls before its accumulating kernel (K8)
        self.replicas = []
        self.active = 0
        self.before_accumulate = None
        # deferred SH gradient (begin_deferred): the mode, the pool of [N,3] residue buffers by (N, device), how many of each are
        # handed out, and the views waiting for the flush -- (means3D leaf, shs leaf, the means3D and shs the kernels read, campos,
        # sh_degree, residue); holding the tensors keeps their memory alive until the flush has been issued
        self.deferred = False
        self.deferred_early_flush = True
        self._param_ids = frozenset(id(p) for p in self.params)
        self.residue_pool_size = SH_FLUSH_MAX_VIEWS
        self._residues = {}
        self._residues_used = {}
        self._pending_sh = []
        self.sh_flushes = 0             # texgs_sh_flush launches so far

    # ---- deferred SH gradient -------------------------------------------------------------------------------------------------
    # K8 re-reads a Gaussian's 45 SH coefficients and read-modify-writes its 45 dL/dSH floats for every view, to add a rank-1
    # product of 15 basis values and the 3 floats of dL/dvd.  Inside ViewPipeline.run the bucket is read only after the last view,
    # so K8 stores those 3 floats (the "residue") and one texgs_sh_flush per step touches the rows once.

    def begin_deferred(self, early_flush=True):
        """Enter the deferred mode (ViewPipeline.run, at its start).  early_flush=False: a full residue pool grows instead of
        flushing in the middle of the step (order="none": nothing orders a stream's flush against the other streams' K8)."""
        assert not self._pending_sh, "begin_deferred with views pending: flush_deferred first"
        self.deferred = True
        self.deferred_early_flush = bool(early_flush)

    def wants_deferred(self, means3D, shs):
        """True when the backward of a view with these inputs should defer: the mode is on and BOTH tensors are sunk into the bucket"""
        if not self.deferred or means3D is None or shs is None or means3D is shs:
            return False
        ids = self._param_ids
        return id(means3D) in ids and id(shs) in ids and shs.dim() == 3 and shs.shape[1] >= 1

    def deferred_pool_full(self, means3D):
        key = (means3D.shape[0], means3D.device)
        return self.deferred_early_flush and self._residues_used.get(key, 0) >= self.residue_pool_size

    def sh_residue_for(self, leaf_means3D, leaf_shs, means3D, shs, campos, sh_degree):
        """An [N,3] residue buffer for K8 (TexGSGrads.dL_dvd_residue) of one view, registered for the flush in call order.
        `leaf_*`: the registered parameters (their slices are the flush's sinks); `means3D`, `shs`, `campos`: the contiguous
        float32 tensors that view's kernels read.  The caller flushes first when deferred_pool_full() (at a point where its
        stream is ordered after the earlier views' K8)."""
        assert self.deferred, "sh_residue_for outside begin_deferred / flush_deferred"
        key = (means3D.shape[0], means3D.device)
        pool = self._residues.setdefault(key, [])
        used = self._residues_used.get(key, 0)
        if used == len(pool):
            pool.append(torch.empty(means3D.shape[0], 3, dtype=torch.float32, device=means3D.device))
        self._residues_used[key] = used + 1
        res = pool[used]
        self._pending_sh.append((leaf_means3D, leaf_shs, means3D, shs, campos, int(sh_degree), res))
        return res

    def _slice_of(self, tensor):
        for p, (off, n) in zip(self.params, self.slices):
            if p is tensor:
                return self.flat[off:off + n]
        raise KeyError("not a registered parameter")

    def flush_pending(self):
        """Issue texgs_sh_flush for the views registered so far, on the current stream, into `flat` (never a replica); the
        residue buffers are free again afterwards (stream order protects them).  The mode stays as it is."""
        pending, self._pending_sh = self._pending_sh, []
        self._residues_used = {}
        if not pending:
            return
        fn = sh_flush_entry()
        k = 0
        while k < len(pending):
            leaf_m, leaf_s, m3, shs = pending[k][:4]
            same = lambda e: e[0] is leaf_m and e[1] is leaf_s and e[2].data_ptr() == m3.data_ptr() and e[3].data_ptr() == shs.data_ptr()
            run = []
            while k < len(pending) and len(run) < SH_FLUSH_MAX_VIEWS and same(pending[k]):
                run.append(pending[k])
                k += 1
            recs = (ShFlushView * len(run))(*[ShFlushView(e[4].data_ptr(), e[6].data_ptr(), e[5], shs.shape[1]) for e in run])
            with _lib.on(m3.device) as stream:
                _lib.call(fn, m3.shape[0], shs.shape[1], m3.data_ptr(), shs.data_ptr(), self._slice_of(leaf_s).data_ptr(),
                          self._slice_of(leaf_m).data_ptr(), recs, len(run), stream)
            self.sh_flushes += 1

    def flush_deferred(self):
        """Leave the deferred mode (ViewPipeline.run, in its `finally`, after the streams are joined and the replicas folded):
        whatever is pending is flushed on the current stream; afterwards .grad of shs and means3D is complete."""
        try:
            self.flush_pending()
        finally:
            self.deferred = False
            self._pending_sh = []
            self._residues_used = {}

    def _assert_flushed(self, what, segment=None):
        """Nothing may read or clear gradients that the flush has not completed.  `segment` = (offset, count): only that run of the flat
        buffer is about to be read -- the texture segment is all-reduced from inside the last view's backward (texture_ready), with
        every view's SH part still pending, and that is fine: the flush adds into the shs and means3D slices alone."""
        if not self._pending_sh:
            return
        if segment is not None:
            lo, hi = segment[0], segment[0] + segment[1]
            slices = {id(p): sl for p, sl in zip(self.params, self.slices)}
            touched = any(off < hi and lo < off + n for e in self._pending_sh for off, n in (slices[id(e[0])], slices[id(e[1])]))
            if not touched:
                return
        raise AssertionError(f"GradBucket.{what} with deferred SH gradients pending: flush_deferred() first")

    def select(self, k: int):
        """Accumulate the following views into buffer k (0 = `flat`, the one .grad aliases; k > 0 = a private replica,
        zero-filled when first made and after every fold()).  Lets views on different streams accumulate with no ordering
        between them; fold() adds the replicas into `flat` before anything reads .grad."""
        while len(self.replicas) < k:
            self.replicas.append(torch.zeros_like(self.flat))
        self.active = k

    def fold(self):
        self.active = 0
        for r in self.replicas:
            self.flat.add_(r)
            r.zero_()

    def sink_for(self, tensor):
        """The bucket slice backing `tensor`'s gradient if `tensor` is one of the registered leaves AND its .grad still
        aliases that slice, else None (autograd then delivers the gradient the normal way).

        `optimizer.zero_grad(set_to_none=True)` -- the PyTorch default and what the reference's optimize_step does
        (models/texture_gaussian3d.py:442-444) -- sets p.grad = None: the slice is then zeroed and re-attached (the
        semantics of "no gradient yet"), so kernels that accumulate into it are never writing into a buffer the
        optimizer no longer sees.  A .grad replaced by some other tensor is left alone (returns None)."""
        for p, (off, n) in zip(self.params, self.slices):
            if p is tensor:
                sl = self.flat[off:off + n]
                if p.grad is None:
                    sl.zero_()
                    p.grad = sl.view_as(p)
                elif p.grad.data_ptr() != self.flat.data_ptr() + 4 * off or not p.grad.is_contiguous():
                    return None
                return sl if self.active == 0 else self.replicas[self.active - 1][off:off + n]
        return None

    def zero(self):
        self._assert_flushed("zero")
        self.flat.zero_()
        for p, (off, n) in zip(self.params, self.slices):   # re-attach if something replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * off:
                p.grad = self.flat[off:off + n].view_as(p)

    def segment_of(self, tensors) -> tuple:
        """(offset, count) of the contiguous run of the flat buffer that backs `tensors` (registered parameters that are adjacent
        in the order the bucket was built with) -- e.g. the texture as one segment and everything else as the other."""
        idx = sorted(i for i, p in enumerate(self.params) if any(p is t for t in tensors))
        if not idx or idx != list(range(idx[0], idx[-1] + 1)):
            raise ValueError("the tensors of a segment must be registered parameters that are adjacent in the bucket")
        off = self.slices[idx[0]][0]
        return off, self.slices[idx[-1]][0] + self.slices[idx[-1]][1] - off

    def all_reduce_async(self, dist, segment=None, after=(), timing=False, wire_dtype=None):
        """Issue the SUM all-reduce of `segment` = (offset, count) of the flat buffer (default: all of it) on the bucket's side
        stream, ordered after the current stream's work so far and after the events in `after`; returns immediately.  Collectives
        are issued in call order on that one stream, so every rank must call this in the same order.  wait() joins.
        Backend "nccl" (= RCCL): in place on the device buffer.  Any other backend (gloo: the CPU tests, and the single-GPU
        rehearsal where two ranks share a device) cannot run asynchronously: the segment is reduced here and now through a host copy.

        `wire_dtype=torch.bfloat16` (opt-in, the wire-size lever of DESIGN.md section 7): the segment travels -- and is SUMMED by the
        collective -- as bf16: half the bytes over xGMI, ~2^-8 relative rounding per partial sum (a segment whose consumer tolerates
        that: the 45 view-dependent SH coefficients per Gaussian are 54 of the 150 MB of a C3 bucket and feed Adam, which normalises
        by the gradient's own running magnitude).  The fp32 buffer is converted into a staging tensor on the comm stream, reduced,
        and converted back in place."""
        off, n = segment if segment is not None else (0, self.flat.numel())
        self._assert_flushed("all_reduce_async", (off, n))
        buf = self.flat[off:off + n]
        if dist.get_backend() != "nccl" or not self.flat.is_cuda:
            for ev in after:                    # (other streams' texture-gradient kernels: the host copy must see their sums)
                ev.synchronize()
            self._reduce_now(dist, buf, wire_dtype)
            return self
        cur = torch.cuda.current_stream(self.flat.device)
        if getattr(self, "_comm", None) is None:
            self._comm = torch.cuda.Stream(self.flat.device)
            self._comm_events = []
        self._comm.wait_stream(cur)
        for ev in after:
            self._comm.wait_event(ev)
        with torch.cuda.stream(self._comm):
            e0 = e1 = None
            if timing:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self._comm)
            if wire_dtype is None or wire_dtype == torch.float32:
                dist.all_reduce(buf, op=dist.ReduceOp.SUM)
                wire_bytes = n * 4
            else:
                stage = buf.to(wire_dtype)      # (allocated on the comm stream: the caching allocator keeps it there)
                dist.all_reduce(stage, op=dist.ReduceOp.SUM)
                buf.copy_(stage)
                wire_bytes = n * stage.element_size()
            if timing:
                e1.record(self._comm)
                self._comm_events.append((wire_bytes, e0, e1))
        self._pending = True
        return self

    def wait(self):
        """Make the current stream wait for every all-reduce issued with all_reduce_async (before the optimizer / zero())."""
        self._assert_flushed("wait")
        if getattr(self, "_pending", False):
            torch.cuda.current_stream(self.flat.device).wait_stream(self._comm)
            self._pending = False
        return self.flat

    def comm_timings(self):
        """[(bytes, milliseconds)] of the timed asynchronous all-reduces so far (synchronises their events); clears the list."""
        out = []
        for nbytes, e0, e1 in getattr(self, "_comm_events", []):
            e1.synchronize()
            out.append((nbytes, e0.elapsed_time(e1)))
        if getattr(self, "_comm_events", None):
            self._comm_events.clear()
        return out

    def _reduce_now(self, dist, buf, wire_dtype=None):
        wd = torch.float32 if wire_dtype is None else wire_dtype
        if buf.is_cuda:
            host = torch.empty(buf.shape, dtype=wd).pin_memory()
            host.copy_(buf, non_blocking=True)
            torch.cuda.current_stream(buf.device).synchronize()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            buf.copy_(host, non_blocking=True)
        elif wd != torch.float32:
            stage = buf.to(wd)
            dist.all_reduce(stage, op=dist.ReduceOp.SUM)
            buf.copy_(stage)
        else:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)

    def all_reduce(self, dist, average_over: int = 0):
        """SUM over ranks (one collective).  average_over > 0 divides by that count afterwards (mean-of-views).

        Backend "nccl" (= RCCL over xGMI) reduces the device buffer in place.  Any other backend (gloo: the CPU tests, and
        the single-GPU rehearsal where two ranks share one device -- RCCL refuses that) goes through a pinned host copy."""
        self._assert_flushed("all_reduce")
        if dist.get_backend() == "nccl":
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
        else:
            if self.flat.is_cuda:
                if getattr(self, "_host", None) is None:
                    self._host = torch.empty(self.flat.shape, dtype=torch.float32).pin_memory()
                self._host.copy_(self.flat, non_blocking=True)
                torch.cuda.current_stream(self.flat.device).synchronize()
                dist.all_reduce(self._host, op=dist.ReduceOp.SUM)
                self.flat.copy_(self._host, non_blocking=True)
            else:
                dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
        if average_over:
            self.flat.div_(float(average_over))
        return self.flat


class ViewPipeline:
    """The views of one multi-view step on `depth` HIP streams (default 2), round-robin.

    Inside one view every kernel depends on the one before it: K1..K5 are fourteen small launches that never fill the chip,
    K6 and K7 end in a tail, and the host waits once per forward for the instance count.  Views are independent of each other,
    so view i+1 is issued on another stream and fills the holes of view i (C3 on one MI355X: 656 -> 772 views/s with three
    streams; K7 itself leaves no room on a CU it occupies, so the gain is the small kernels and the tails).  Ordering that
    remains:

    * K8 of view i+1 waits for the whole backward of view i (`order="accumulate"`, the default with a GradBucket sink): K8
      adds into the shared gradient sink with plain read-modify-writes; K7 and the texture-gradient reduce only use atomics
      and per-stream scratch and run unordered.  Everything autograd does downstream of the rasterizer node (AccumulateGrad
      of gradients that are not in the sink) is issued after that K8 on the same stream, hence ordered too; gradient paths
      that bypass the rasterizer are the caller's to order (`order="backward"` serialises whole backwards);
    * a stream runs its own views in order, so per-stream scratch (moment accumulators, texture bins: keyed by stream in
      texgs.rasterizer) is never shared by two views in flight;
    * the caller's stream is joined before (parameters, zeroed sinks) and after (all-reduce, optimizer).

    `forward_fn(view)` runs the forward and whatever loss is attached and returns what `backward_fn` needs;
    `backward_fn(obj)` calls autograd (which runs each node on the stream its forward ran on)."""

    def __init__(self, device, depth: int = 2):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.device = torch.device(device)
        self.streams = [torch.cuda.Stream(self.device) for _ in range(depth)] if depth > 1 else []

    def close(self):
        """Free the backward scratch (moment accumulators, texture-gradient bins) cached for this pipeline's streams."""
        from . import rasterizer
        for s in self.streams:
            s.synchronize()
            rasterizer.release_scratch(self.device, s.cuda_stream)
        self.streams = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prefetch_batched(self, views, prefetch_fn, stream_of, batch):
        """The batched front end (texgs.rasterizer.batched_prefetch): prefetch_fn is called for EVERY view of the step now, under the
        stream the view will run on, inside a batch scope -- where the rasterizer's prefetch only registers --, and the views that can
        share K1..K5 run them once, on the current stream.  -> per view: True = nothing is left to prefetch for it; False = the caller
        prefetches it in its usual rhythm (it fitted no group, or batching is off: `batch` false, no prefetch_fn, fewer than two views,
        a pipeline that is not on a GPU)."""
        if not batch or prefetch_fn is None or len(views) < 2 or self.device.type != "cuda":
            return [False] * len(views)
        from . import rasterizer
        owned = []
        with rasterizer.batched_prefetch(begin_rest=False) as scope:
            for i, v in enumerate(views):
                n0 = len(scope.requests)
                with stream_of(i):
                    prefetch_fn(v)
                owned.append(scope.requests[n0:])
        return [all(r.batched for r in reqs) for reqs in owned]      # (a prefetch_fn that registered nothing has done its work already)

    def run(self, views, forward_fn, backward_fn=None, sink=None, order="accumulate", texture_ready=None, prefetch_fn=None,
            prefetch_ahead=1, batch=True):
        """`prefetch_fn(view)` (optional; e.g. GaussianRasterizer.prefetch with the arguments forward_fn will use): begins the forward
        of the view this stream renders NEXT -- K1 and the instance-count readback -- right after the current view's forward and
        BEFORE its backward is queued, so that the next forward on this stream does not wait for that backward (the first view of every
        stream is begun before the loop).  The host then runs up to one view per stream ahead of the device instead of none, which is
        what keeps the queues full when a host thread is descheduled for a few milliseconds.

        `texture_ready(events)` (optional, needs a GradBucket sink and order="accumulate"): called ONCE, from inside the last
        view's backward, between its K7 + texture-gradient reduce and its K8 -- the point where every view's contribution to
        dL/dtexture has been issued; `events` = one event per stream, recorded after that stream's latest K7 + reduce.  The caller
        starts the texture segment's all-reduce there (GradBucket.all_reduce_async(..., after=events)).

        order (what of view i+1 waits for view i when both add into `sink`):
        "backward"   -- its whole backward (works with any gradient path, e.g. plain autograd accumulation);
        "accumulate" -- only its accumulating kernel K8, through sink.before_accumulate (needs a GradBucket sink);
        "none"       -- nothing: every stream accumulates into its own replica of the bucket, folded at the end.

        `batch` (default on; needs prefetch_fn): the batched front end -- every view's forward is registered through prefetch_fn
        BEFORE the loop and the views with the same inputs, image size and sh_degree run K1..K5 once for all of them on the caller's
        stream (texgs.rasterizer.batched_prefetch); their forwards in the loop are K6 alone.  Views that fit no group keep the rhythm
        above.  batch=False: every view takes the per-view path."""
        results = []
        views = list(views)
        # the deferred SH gradient of a GradBucket (a sink without these two methods is driven exactly as before)
        begin_deferred = getattr(sink, "begin_deferred", None) if backward_fn is not None else None
        flush_deferred = getattr(sink, "flush_deferred", None) if begin_deferred is not None else None
        if not self.streams:                       # depth 1: the caller's stream, nothing to order
            if flush_deferred is not None:
                begin_deferred()
            try:
                batched = self._prefetch_batched(views, prefetch_fn, lambda i: contextlib.nullcontext(), batch)
                for i, v in enumerate(views):
                    obj = forward_fn(v)
                    if prefetch_fn is not None and i + 1 < len(views) and not batched[i + 1]:
                        prefetch_fn(views[i + 1])
                    if backward_fn is not None:
                        if texture_ready is not None and sink is not None and i == len(views) - 1:
                            sink.before_accumulate = lambda: texture_ready([])
                        try:
                            backward_fn(obj)
                        finally:
                            if sink is not None:
                                sink.before_accumulate = None
                    results.append(obj)
            finally:
                if flush_deferred is not None:
                    flush_deferred()
            return results
        if order not in ("backward", "accumulate", "none"):
            raise ValueError(order)
        if sink is None and order != "backward":
            order = "backward"
        cur = torch.cuda.current_stream(self.device)
        if flush_deferred is not None:
            begin_deferred(early_flush=order != "none")
        prev_bwd = None
        render_done = {}                            # stream index -> event after that stream's latest K7 + texture-gradient reduce
        depth = len(self.streams)
        try:
            # the batched front end: K1..K5 of every view that can share them, once, on the caller's stream, before the streams fork
            batched = self._prefetch_batched(views, prefetch_fn, lambda i: torch.cuda.stream(self.streams[i % depth]), batch)
            for s in self.streams:
                s.wait_stream(cur)
            ahead = depth * max(1, int(prefetch_ahead))     # (views; prefetch_ahead = forwards begun ahead PER STREAM)
            if prefetch_fn is not None:
                for i, v in enumerate(views[:ahead]):
                    if not batched[i]:
                        with torch.cuda.stream(self.streams[i % depth]):
                            prefetch_fn(v)
            for i, v in enumerate(views):
                k = i % depth
                s = self.streams[k]
                with torch.cuda.stream(s):
                    if order == "none":
                        sink.select(k)
                    obj = forward_fn(v)
                    if prefetch_fn is not None and i + ahead < len(views) and not batched[i + ahead]:
                        prefetch_fn(views[i + ahead])
                    if backward_fn is not None:
                        if order == "backward" and prev_bwd is not None:
                            s.wait_event(prev_bwd)
                        if order == "accumulate":
                            last = i == len(views) - 1

                            def hook(ev=prev_bwd, s=s, k=k, last=last):
                                if texture_ready is not None:
                                    e = torch.cuda.Event()
                                    e.record(s)
                                    render_done[k] = e
                                    if last:
                                        texture_ready([render_done[j] for j in sorted(render_done)])
                                if ev is not None:
                                    s.wait_event(ev)
                            sink.before_accumulate = hook
                        backward_fn(obj)
                        prev_bwd = torch.cuda.Event()
                        prev_bwd.record(s)
                results.append(obj)
        finally:
            if sink is not None:
                sink.before_accumulate = None
            for s in self.streams:
                cur.wait_stream(s)
            if sink is not None and order == "none":
                sink.fold()
            if flush_deferred is not None:          # on the caller's stream, which has just been joined with every stream: no new wait
                flush_deferred()
        return results
