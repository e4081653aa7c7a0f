"""Host side of the textured Gaussian rasterizer: torch.autograd.Function over the C ABI of libtexgs.so.

Mirrors the operator surface the reference imports at render/uv_tex_render.py:4 and calls at :25-38, :40,
:56-66 (GaussianRasterizationSettings / GaussianRasterizer): same names, argument meaning and 6-tuple return.
PyTorch is plumbing here (device memory through the caching allocator, the current HIP stream, autograd
bookkeeping); all arithmetic runs in the hand-written gfx950 kernels.
"""
import ctypes as C
import math
import os as _os
import threading as _threading
import weakref as _weakref
from collections import namedtuple
from types import SimpleNamespace
from typing import NamedTuple

import torch
from torch import nn

from . import _lib

USE_TEX_BINS = _os.environ.get("TEXGS_TEX_BINS", "1") != "0"       # binned two-pass texture gradient
TEX_REC_CAP = int(_os.environ.get("TEXGS_REC_CAP", "0"))           # fixed record capacity (tests); 0 = adaptive
# OPT-IN fast path: add into a leaf's existing .grad in place instead of handing autograd a temporary.  Off by default because
# it is not what autograd does: torch.autograd.grad() would then mutate .grad, and tensor hooks / post-accumulate-grad hooks /
# DDP reducer hooks on those leaves would not fire (leaves that carry hooks are skipped even when it is on).  The supported fused
# path is an explicit texgs.multiview.GradBucket sink.
DIRECT_LEAF_GRADS = _os.environ.get("TEXGS_DIRECT_LEAF_GRADS", "0") != "0"
# upper bound of ONE record buffer; there is one per (device, stream) that runs backwards (a depth-3 ViewPipeline holds three)
TEX_REC_BYTES_MAX = int(float(_os.environ.get("TEXGS_BIN_GB_MAX", "4")) * (1 << 30))
# per-Gaussian gradient outputs in the order / bit positions of TEXGS_ACC_* (texgs.h)
_ACC_BITS = dict(means3D=1, means2D=2, shs=4, opacities=8, scales=16, rotations=32, uvs=64, color_offset=128, cov3D=256)


class GaussianRasterizationSettings(NamedTuple):
    """Field names and order = keywords at render/uv_tex_render.py:25-38."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


_ptr = _lib.ptr         # bound once: a view's forward and backward take about forty pointers


def _f32c(t: torch.Tensor, name: str, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


class _Arena:
    """One device allocation carved into named, 256-byte-aligned pieces."""

    def __init__(self, device):
        self.device, self.specs, self.size, self.buf = device, {}, 0, None

    def add(self, name, shape, dtype):
        off = (self.size + 255) & ~255
        self.specs[name] = (off, tuple(shape), dtype)
        self.size = off + math.prod(shape) * dtype.itemsize

    def commit(self):
        self.buf = torch.empty(max(self.size, 1), dtype=torch.uint8, device=self.device)

    def place(self, step_buffer, offset):
        """Instead of commit(): the pieces live at `offset` (a multiple of 256) of a _StepBuffer shared with other arenas, which this
        arena keeps alive."""
        assert offset % 256 == 0 and offset + self.size <= step_buffer.buf.numel()
        self.buf, self.owner = step_buffer.buf[offset:offset + max(self.size, 1)], step_buffer

    def ptr(self, name):
        return self.buf.data_ptr() + self.specs[name][0] if name in self.specs else None

    def view(self, name):
        off, shape, dtype = self.specs[name]
        return self.buf[off:off + math.prod(shape) * dtype.itemsize].view(dtype).view(shape)


class _Tensors(dict):
    """What a forward leaves behind, by name: real tensors (inputs kept alive, outputs) plus views into the arenas, made on
    first access.  A name that was not allocated (e.g. the survivor lists of a forward-only call) reads as None."""

    def __init__(self, arenas, **real):
        super().__init__(**real)
        self._arenas = arenas

    def __missing__(self, name):
        for ar in self._arenas:
            if name in ar.specs:
                self[name] = v = ar.view(name)
                return v
        self[name] = None
        return None

    def get(self, name, default=None):
        v = self[name]
        return default if v is None else v


# Two forwards of the same geometry share the tile binning and K6's survivor lists (the reference renders every training view
# twice: models/texture_gaussian3d.py:318 and :375-389 -- same camera, same Gaussians, sh_degree 0 the second time; visual_step
# :499-511 likewise).  Decided by K1's geometry fingerprint (texgs.h texgs_num_rendered_reduce), so recomputed activations
# (sigmoid / exp outputs are new tensors on every render() call) share too.  One entry per (device, stream).
GEOM_CACHE = _os.environ.get("TEXGS_GEOM_CACHE", "1") != "0"
_CAPACITY_HINT = {}
_GEOM = {}                  # (device index, stream) -> _GeomEntry of the last forward that built lists there
_GeomEntry = namedtuple("_GeomEntry", "ints cam_key fingerprint D cap bin arenas handoff counts")
_GEOM_STATS = {"hits": 0, "misses": 0, "late_handoffs": 0}
# A forward that autograd may or may not differentiate (retexture.py:27 / visual_step build a graph and never call backward)
# leaves K6's hand-off to the backward once two graphs in a row were dropped unused; the first backward that does arrive
# produces the hand-off itself (one more K6) and switches the forwards back.
# The predictor: autograd forwards are numbered; per device, the highest number whose backward ran and the numbers of
# those dropped without one.  (Order-independent: a state that the garbage collector frees late cannot reset the streak.)
_SERIAL = [0]
_LAST_DIFFERENTIATED = {}
_DROPPED = {}
_PRED_LOCK = _threading.RLock()       # the predictor's dicts are touched from __del__ (any thread, any time the collector runs)


def unused_streak(dev_index):
    """Autograd forwards on this device that were dropped without a backward since the last one that was differentiated."""
    with _PRED_LOCK:
        last = _LAST_DIFFERENTIATED.get(dev_index, -1)
        return sum(1 for n in _DROPPED.get(dev_index, ()) if n > last)


def reset_handoff_predictor():
    with _PRED_LOCK:
        _LAST_DIFFERENTIATED.clear()
        _DROPPED.clear()


def geometry_cache_stats():
    """{'hits': n, 'misses': n} of the shared-geometry path since import (diagnostics / tests)."""
    return dict(_GEOM_STATS)


# Backward scratch, ONE entry per (device, HIP stream): the moment accumulators (grow-only, sliced [:N]; all-zero between
# calls: K8 clears what it read) and the texture-gradient bins of the last resolution used on that stream.  A stream runs
# its views in order, so its scratch is never shared by two views in flight.  release_scratch() drops entries (ViewPipeline
# does that for its streams when it is closed / collected).
_SCRATCH = {}


def release_scratch(device=None, stream=None):
    """Free the backward scratch and the shared-geometry entry cached for (device, stream); None = every device / stream."""
    for cache in (_SCRATCH, _GEOM, _PREFETCH):
        for key in list(cache):
            if (device is None or key[0] == torch.device(device).index) and (stream is None or key[1] == int(stream)):
                for _, fwd in (cache[key] if cache is _PREFETCH else ()):
                    fwd.abandon()
                del cache[key]


def scratch_bytes():
    """Bytes currently held by the module's caches (diagnostics / tests): the backward scratch per (device, stream) and the arenas
    the shared-geometry entries keep alive (the last list-building forward of every (device, stream))."""
    total = 0
    for sc in _SCRATCH.values():
        if sc.acc is not None:
            total += sc.acc.numel() * 4
        if sc.bins is not None:
            total += sc.bins.nbytes()
    for e in _GEOM.values():
        total += sum(ar.buf.numel() for ar in e.arenas if ar is not None and ar.buf is not None)
    return total + step_buffer_bytes()


class _StepBuffer:
    """One device allocation that holds the K1..K5 outputs of ALL views of a batched front end (batched_prefetch): every view's arenas
    are slices of it (_Arena.place) and keep it alive -- from the start of the step until the last of its views has run its backward
    (or was dropped: release_scratch abandons the pending ones).  A step has two: one sized by V and N, made before K1, and one sized
    by the sum of the views' instance counts, made when those have been read back."""

    def __init__(self, nbytes, device):
        self.buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _STEP_BUFFERS.add(self)


_STEP_BUFFERS = _weakref.WeakSet()


def step_buffer_bytes():
    """Bytes of the batched front end's step buffers that are alive now (counted in scratch_bytes())"""
    return sum(b.buf.numel() for b in list(_STEP_BUFFERS))


class _TexBins:
    """Scratch of the binned texture gradient for one (device, R, stream): the record buffer (TexGSGrads.tex_bins, 16 bytes per
    bilinear footprint of a view, exactly-sized contiguous lists), the per-bin fill cursors + two status words (all-zero
    between calls: the reduce kernel clears what it read) and the list offsets of the call in flight.  The buffer grows to
    what the views need: every call leaves the number of records its lists wanted in the word after the cursors; it is copied
    to pinned host memory asynchronously every few calls and looked at only when that copy has completed -- the backward
    never waits for it.  A buffer that is too small is not an error (what does not fit goes through atomics), so a stale
    size costs speed, never correctness."""

    def __init__(self, lib, device, R):
        self.device, self.R = device, R
        self.nbins = int(lib.texgs_tex_bin_count(R))
        self.cursor = torch.zeros(self.nbins + 2, dtype=torch.int32, device=device)
        self.base = torch.empty(2 * self.nbins + 1, dtype=torch.int32, device=device)      # list offsets, then the reduce launch order
        self.cap = 0
        self.rec = None
        self.host_stat = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None
        self.calls = 0

    def nbytes(self):
        return ((0 if self.rec is None else self.rec.numel()) + self.cursor.numel() + self.base.numel()) * 4

    def _resize(self, cap):
        cap = max(1024, min(int(cap), TEX_REC_BYTES_MAX // (4 * _lib.TEXBIN_RECORD_FLOATS)))
        if cap != self.cap:
            self.rec = None
            self.rec = torch.empty(cap * _lib.TEXBIN_RECORD_FLOATS, dtype=torch.float32, device=self.device)
            self.cap = cap

    def before_call(self, D, counts=None):
        if TEX_REC_CAP:
            self._resize(TEX_REC_CAP)
            return
        if self.rec is None and counts is not None and not torch.cuda.is_current_stream_capturing():
            # FIRST backward on this (device, stream) -- and the first after release_scratch(): size the buffer from K6's exact
            # per-bin counts.  This is ONE blocking device->host read (ADVICE r5 asked to remove or document it): it waits for this
            # view's forward, which the backward is ordered behind anyway; afterwards the asynchronous statistic below adapts the
            # size and nothing here ever waits again.  A guess from D instead (tried: 24 records per instance) sends the excess
            # of large-splat scenes through atomics on exactly the calls tests and benchmarks look at first, and makes the first
            # call take another path than the following ones.  Under stream capture: the guess below, no read.
            self._resize(int(counts.sum().item() * 1.25) + 4096)
        if self.event is not None and self.event.query():
            self.event = None
            wanted = int(self.host_stat[0])
            if wanted > self.cap:
                self._resize(int(wanted * 1.25) + 4096)
        if self.rec is None:
            self._resize(24 * max(int(D), 1024))        # first guess: ~17 contributing pixels per (tile, Gaussian) instance at C3

    def after_call(self):
        self.calls += 1
        if self.event is None and not TEX_REC_CAP and (self.calls <= 4 or self.calls % 16 == 0):
            self.host_stat.copy_(self.cursor[self.nbins:self.nbins + 1], non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(self.device))


class _State:
    """Everything one forward leaves behind for its backward (per call: no global scratch, two forwards may
    be alive before a backward, models/texture_gaussian3d.py:318,378,410)."""
    __slots__ = ("frame", "inputs", "geom", "bin", "img", "tensors", "args", "N", "K", "R", "H", "W", "D", "cap", "tiles",
                 "want_counts", "lazy", "backward_ran", "shared_geometry", "serial", "fingerprint", "__weakref__")

    def __init__(self, frame, inputs, geom, bin, img, tensors, args, D, cap, tiles, want_counts, lazy, shared_geometry):
        self.frame, self.inputs, self.geom, self.bin, self.img, self.tensors, self.args = frame, inputs, geom, bin, img, tensors, args
        self.N, self.K, self.R, self.H, self.W = args.N, args.K, args.R, frame.image_height, frame.image_width
        self.D, self.cap, self.tiles = D, cap, tiles
        self.want_counts, self.lazy, self.backward_ran, self.shared_geometry = want_counts, lazy, False, shared_geometry
        self.fingerprint = None     # K1's geometry fingerprint of this forward (set by the forward; diagnostics / tests)
        with _PRED_LOCK:
            _SERIAL[0] += 1
            self.serial = _SERIAL[0]

    def __del__(self):          # the forwards' hand-off predictor: was this autograd forward ever differentiated?
        try:
            if getattr(self, "lazy", False) and not self.backward_ran:
                dev = self.args.means3D.device.index
                with _PRED_LOCK:
                    last = _LAST_DIFFERENTIATED.get(dev, -1)
                    _DROPPED[dev] = [n for n in _DROPPED.get(dev, []) if n > last][-8:] + [self.serial]
        except Exception:
            pass


def _make_frame(st: GaussianRasterizationSettings, N, K, R, device, keep):
    bg = _f32c(st.bg, "bg", device).reshape(-1)
    vm = _f32c(st.viewmatrix, "viewmatrix", device).reshape(-1)
    pm = _f32c(st.projmatrix, "projmatrix", device).reshape(-1)
    cp = _f32c(st.campos, "campos", device).reshape(-1)
    if bg.numel() != 3 or vm.numel() != 16 or pm.numel() != 16 or cp.numel() != 3:
        raise ValueError("bg/campos must have 3 elements and viewmatrix/projmatrix 16")
    keep.extend([bg, vm, pm, cp])
    return _lib.Frame(int(st.image_height), int(st.image_width), float(st.tanfovx), float(st.tanfovy), float(st.scale_modifier),
                      int(st.sh_degree), int(K), int(R), int(N), 1 if st.debug else 0, _ptr(bg), _ptr(vm), _ptr(pm), _ptr(cp))


# ---- forward prefetch: K1 (+ the D readback, + K2) of a LATER view issued early ---------------------------------------------------
# A forward waits once for the device: D, the instance count that sizes K3..K6's launches.  On a stream that runs its views in order,
# that wait is for everything the stream still has queued -- the previous view's whole backward.  With a few views pipelined over a
# few streams the GPU stays busy meanwhile, but the host is then never more than a view or two ahead of the device: any host thread
# stall of a few milliseconds (a neighbour process on the box's cores) drains the queue.  prefetch_forward issues K1 and the readback
# of a view AHEAD of the backward that is about to be queued on the same stream; when that view's forward is called, with the same
# tensors (same storage, same version counters) and settings, its D arrived long ago and nothing waits.  One pending forward per key;
# a forward that does not match anything pending runs as usual.
_PREFETCH = {}             # (device index, stream) -> [(key, _Forward that has begun)]; a stream without pending forwards has no entry
_PIN_POOL = {}             # words -> [pinned int32 tensors]


def _pin_take(words):
    pool = _PIN_POOL.setdefault(words, [])
    return pool.pop() if pool else torch.empty(max(words, 1), dtype=torch.int32).pin_memory()


def _pin_give(t):
    pool = _PIN_POOL.setdefault(t.numel(), [])
    if len(pool) < 16:
        pool.append(t)


def _prefetch_take(device, key):
    skey = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    lst = _PREFETCH.get(skey, ())
    for k, (key_k, fwd) in enumerate(lst):
        if key_k == key:
            del lst[k]
            if not lst:
                del _PREFETCH[skey]
            return fwd


# a forward's inputs after _check_inputs: contiguous float32 tensors (None where absent) and the sizes they imply
_Args = namedtuple("_Args", "means3D shs opacities scales rotations uvs gradient_uvs texture color_offset cov3D_precomp N K R")
# TexGSImage's K6 -> K7 hand-off pointers; the arena pieces (_add_handoff) carry the same names
_HANDOFF = tuple(n for n, _ in _lib.Image._fields_[6:])


def _check_inputs(st, means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset=None, cov3D_precomp=None):
    """Types, dtypes, shapes and devices of a forward's inputs -> _Args.  Pure: no library call, tensors of any one device."""
    device = means3D.device
    N = means3D.shape[0]
    means3D = _f32c(means3D, "means3D", device)
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError("means3D must be [N,3]")
    opacities = _f32c(opacities, "opacities", device)
    if opacities.numel() != N:
        raise ValueError(f"per-Gaussian inputs must have exactly N rows (N={N}; opacities {tuple(opacities.shape)})")
    if cov3D_precomp is not None:
        if texture is not None:
            raise ValueError("cov3D_precomp is an input of the untextured surface only")
        cov3D_precomp = _f32c(cov3D_precomp, "cov3D_precomp", device)
        if cov3D_precomp.shape != (N, 6):
            raise ValueError(f"cov3D_precomp must be [N,6], got {tuple(cov3D_precomp.shape)}")
        scales = rotations = None
    else:
        scales = _f32c(scales, "scales", device)
        rotations = _f32c(rotations, "rotations", device)
        if scales.shape != (N, 3) or rotations.shape != (N, 4):
            raise ValueError("per-Gaussian inputs must have exactly N rows "
                             f"(N={N}; scales {tuple(scales.shape)}, rotations {tuple(rotations.shape)})")
    if texture is not None:
        uvs = _f32c(uvs, "uvs", device)
        gradient_uvs = _f32c(gradient_uvs, "gradient_uvs", device)
        texture = _f32c(texture, "texture", device)
        if uvs.shape != (N, 3) or gradient_uvs.numel() != 9 * N:
            raise ValueError("per-Gaussian inputs must have exactly N rows "
                             f"(N={N}; uvs {tuple(uvs.shape)}, gradient_uvs {tuple(gradient_uvs.shape)})")
        if texture.dim() != 4 or texture.shape[0] != 6 or texture.shape[1] != texture.shape[2] or texture.shape[3] != 3:
            raise ValueError(f"texture must be [6,R,R,3], got {tuple(texture.shape)}")
        R = texture.shape[1]
    else:
        uvs = gradient_uvs = None
        R = 1
    K = 0
    if shs is not None:
        shs = _f32c(shs, "shs", device)
        if shs.dim() != 3 or shs.shape[0] != N or shs.shape[2] != 3:
            raise ValueError(f"shs must be [N,K,3], got {tuple(shs.shape)}")
        K = shs.shape[1]
        if K > 15:
            raise ValueError("shs holds at most 15 view-dependent coefficients (degree 3)")
    if color_offset is not None:
        color_offset = _f32c(color_offset, "color_offset", device)
        if color_offset.shape != (N, 3):
            raise ValueError(f"color_offset must be [N,3], got {tuple(color_offset.shape)}")
    if int(st.sh_degree) < 0 or int(st.sh_degree) > 3:
        raise ValueError("sh_degree must be in [0,3]")
    return _Args(means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset, cov3D_precomp, N, K, R)


def _add_handoff(ar, cap, tiles, R, want_counts):
    """The K6 -> K7 hand-off of the per-block survivor lists, laid out in this ONE place: the pieces sized by the instance capacity
    (`cap`; None = not in this arena) and the per-tile ones (`tiles`; None = not in this arena)."""
    if cap is not None:         # four blocks per tile, each at most the tile's list length
        ar.add("survivors", (4 * max(cap, 1), 2), torch.int32)
        ar.add("surv_qmask", (4 * max(cap, 1),), torch.int16)
    if tiles is not None:
        ar.add("surv_count", (4 * tiles,), torch.int32)
        if want_counts:
            ar.add("tex_bin_count", (2 * int(_lib.load().texgs_tex_bin_count(R)),), torch.int32)     # reserved | overflow footprints per bin
            ar.add("tex_bin_resv", (4 * tiles, _lib.RESV_WORDS), torch.int32)      # K6's per-block reservations in the record lists


class _Forward:
    """One forward in two steps.  begin(): validation, every allocation, K1, the asynchronous copy of K1's partial sums (D and the
    geometry fingerprint) into pinned memory, an event and -- unless earlier lists are expected to be shared -- K2 behind it.
    finish(): the forward's one host wait, then K3..K6 or the shared-geometry path -> (outputs, _State).  forward_raw runs both back
    to back; a prefetched forward sits in _PREFETCH between them, and abandon() is for one dropped from there unfinished."""

    def __init__(self, st, tensors, for_backward, count_bins, lazy):
        self.st, self.raw, self.flags = st, tensors, (for_backward, count_bins, lazy)

    def key(self):
        """What identifies a begun forward as THE forward of a later call: settings, every tensor's storage / version / shape, flags."""
        t = lambda x: None if x is None else (x.data_ptr(), x._version, tuple(x.shape), x.requires_grad)
        st = self.st
        return (int(st.image_height), int(st.image_width), float(st.tanfovx), float(st.tanfovy), float(st.scale_modifier), int(st.sh_degree),
                bool(st.debug), t(st.bg), t(st.viewmatrix), t(st.projmatrix), t(st.campos)) + tuple(t(x) for x in self.raw) + self.flags

    def begin(self):
        lib = _lib.load()
        self._plan()
        a, N, stream = self.args, self.args.N, self.stream
        with torch.cuda.device(a.means3D.device):
            self.fix.commit()
            self._bind()
            refs = self.refs
            _lib.call(lib.texgs_preprocess_forward, *refs, stream)
            # the one device->host read of a forward, in two steps: the copy into pinned memory is issued here, finish() waits for it
            pin = self.pin = _pin_take(int(lib.texgs_num_rendered_words(N)))
            _lib.call(lib.texgs_num_rendered_begin, refs[2], N, pin.data_ptr(), pin.numel(), 0, stream)
            self.d_ev = torch.cuda.Event()
            self.d_ev.record(self.cur_stream)
            if self.entry is None:      # K2 behind the event: the host waits for K1 + the copy only, the device goes on sorting
                _lib.call(lib.texgs_depth_sort_scan, refs[2], N, stream)
        return self

    def _plan(self, batched=False):
        """Validation and the layout of the arena sized by N and the image (not allocated yet).  `batched`: one of the views of a batched
        front end (_begin_views) -- it builds its own lists whatever the shared-geometry cache holds (the views are different cameras)."""
        lib, st = _lib.load(), self.st
        a = self.args = _check_inputs(st, *self.raw)
        for_backward, count_bins, lazy = self.flags
        device, N = a.means3D.device, a.N
        if count_bins is None:
            count_bins = for_backward
        self.handoff = bool(for_backward) and not (lazy and unused_streak(device.index) >= 2)
        self.want_counts = bool(count_bins and for_backward and a.texture is not None and USE_TEX_BINS)
        H, W = int(st.image_height), int(st.image_width)
        self.tiles = ((W + _lib.TILE - 1) // _lib.TILE) * ((H + _lib.TILE - 1) // _lib.TILE)
        cur_stream = self.cur_stream = torch.cuda.current_stream(device)
        stream = self.stream = cur_stream.cuda_stream
        self.binned = None          # (D, fingerprint, event) once a batched front end has built this view's lists
        self.keep = list(a[:10])
        with torch.cuda.device(device):
            self.frame = _make_frame(st, N, a.K, a.R, device, self.keep)
            self.inputs = _lib.Inputs(*map(_ptr, a[:10]))
            i32, f32, u8, n1 = torch.int32, torch.float32, torch.uint8, max(N, 1)
            # a forward that may share an earlier one's lists: same sizes, same camera tensors -- K1's fingerprint decides
            self.gints = (N, H, W, a.R if a.texture is not None else 0, float(st.tanfovx), float(st.tanfovy), float(st.scale_modifier),
                          a.cov3D_precomp is not None)
            self.cam_key = tuple((t.data_ptr(), t._version) for t in (st.viewmatrix, st.projmatrix, st.campos))
            gkey = self.gkey = (device.index, int(stream))
            entry = _GEOM.get(gkey) if (GEOM_CACHE and not batched) else None
            if entry is not None and not (entry.ints == self.gints and entry.cam_key == self.cam_key):
                del _GEOM[gkey]         # another view / size: the old lists cannot be shared any more -- let go of their arenas before this
                entry = None            # forward allocates its own (they stay alive only while a state that shares them does)
            self.entry = entry          # the candidate to share lists with; None: this forward builds its own
            # Everything the kernels keep between forward and backward lives in TWO allocations (one sized by N / the image, one by
            # the instance capacity): ~20 separate torch.empty calls were ~0.1 ms of host time per view.  Tensor views of the
            # pieces are made on demand (tests, diagnostics).
            scan_bytes = lib.texgs_scan_temp_bytes(N)
            fix = self.fix = _Arena(device)
            fix.add("rec", (n1, _lib.REC_TEST_FLOATS), f32)          # test records: xy, conic, opacity, cull aids
            fix.add("rec_shade", (n1, _lib.REC_SHADE_FLOATS), f32)
            fix.add("depth", (n1,), f32)
            fix.add("rect", (n1, 2), i32)
            fix.add("tiles_touched", (n1,), i32)
            fix.add("offsets", (n1,), i32)
            fix.add("scan_temp", (scan_bytes,), u8)
            fix.add("final_T", (H, W), f32)
            fix.add("n_contrib", (H, W), i32)
            if entry is None:
                self._add_lists(fix)
            self.scan_bytes = scan_bytes

    def _bind(self, batched=False):
        """With the arena in place: the outputs, the structs of the C ABI and -- unless `batched`, where the instance counts are known
        before anything of that size is needed -- the arena sized by the instance capacity."""
        a, st, fix, entry, scan_bytes = self.args, self.st, self.fix, self.entry, self.scan_bytes
        device, N, H, W = a.means3D.device, a.N, int(st.image_height), int(st.image_width)
        i32, f32 = torch.int32, torch.float32
        radii = torch.empty(N, dtype=i32, device=device)          # K1 writes every entry (0 for culled)
        self.geom = _lib.Geom(fix.ptr("rec"), fix.ptr("rec_shade"), fix.ptr("depth"), _ptr(radii), fix.ptr("rect"),
                              fix.ptr("tiles_touched"), fix.ptr("offsets"), fix.ptr("scan_temp"), scan_bytes)
        # everything is allocated BEFORE the one device->host sync, the D-sized buffers from a capacity hint
        # (largest D seen on this device x 1.25): K1 -> sync (K2 runs meanwhile) -> K3..K6 with little host work between
        self.outs = (torch.empty(3, H, W, dtype=f32, device=device), torch.empty(1, H, W, dtype=f32, device=device),
                     torch.empty(3, H, W, dtype=f32, device=device), torch.empty(1, H, W, dtype=f32, device=device), radii)
        self.img = _lib.Image(*map(_ptr, self.outs[:4]), fix.ptr("final_T"), fix.ptr("n_contrib"), None, None, None, None, None)
        self.hint_key = (device.index, N, H, W)
        self.cap = _CAPACITY_HINT.get(self.hint_key, max(4 * N, 1024))
        self.binning = self.bin_ar = None
        if entry is None and not batched:
            self._alloc_bin(self.cap, fix)
        self.refs = [C.byref(x) for x in (self.frame, self.inputs, self.geom)]

    def _add_lists(self, ar):           # per-tile pieces of the lists (a candidate adds them only if it has to build lists after all)
        ar.add("ranges", (self.tiles, 2), torch.int32)              # zero-filled by K3
        ar.add("tile_order", (self.tiles,), torch.int32)
        if self.handoff:
            _add_handoff(ar, None, self.tiles, self.args.R, self.want_counts)

    def _alloc_bin(self, cap, lists_ar, commit=True):
        """The arena sized by the instance capacity; `lists_ar`: where the per-tile pieces are (None: nowhere yet -- they go in here too).
        commit=False: only laid out -- the caller places it in a step buffer and calls _bind_bin."""
        c1, tiles = max(cap, 1), self.tiles
        sort_bytes = _lib.load().texgs_sort_temp_bytes(cap, tiles)
        ar = self.bin_ar = _Arena(self.fix.device)
        ar.add("keys_unsorted", (c1,), torch.int64)
        ar.add("keys_sorted", (c1,), torch.int64)
        ar.add("point_list", (c1,), torch.int32)
        ar.add("sort_temp", (sort_bytes,), torch.uint8)
        if lists_ar is None:
            self._add_lists(ar)
        if self.handoff:
            _add_handoff(ar, cap, None, self.args.R, self.want_counts)
        self.sort_bytes = sort_bytes
        if commit:
            ar.commit()
            self._bind_bin(lists_ar)
        return ar

    def _bind_bin(self, lists_ar):
        ar, sort_bytes = self.bin_ar, self.sort_bytes
        la = lists_ar if lists_ar is not None else ar
        self.binning = _lib.Binning(0, ar.ptr("keys_unsorted"), ar.ptr("keys_sorted"), ar.ptr("point_list"), la.ptr("ranges"),
                                    la.ptr("tile_order"), ar.ptr("sort_temp"), sort_bytes)
        for n in _HANDOFF:
            setattr(self.img, n, (ar if n in ar.specs else la).ptr(n))

    def finish(self):
        lib, a, img, entry, refs = _lib.load(), self.args, self.img, self.entry, self.refs
        for_backward, _, lazy = self.flags
        stream, cap, pin = self.stream, self.cap, self.pin
        if self.binned is not None:
            # a view of a batched front end (_begin_views): K1..K5 ran with the other views' and D was read back there; what is left
            # is K6, on the stream this forward is called on -- ordered behind the batch's launches by their event, whatever that stream is
            D, fp, ready = self.binned
            shared, binning = False, self.binning
            with torch.cuda.device(a.means3D.device):
                cur = torch.cuda.current_stream(a.means3D.device)
                if cur.cuda_stream != stream:
                    cur.wait_event(ready)
                from .multiview import views_entries
                _lib.call(views_entries().render_forward_binned, *refs, C.byref(binning), C.byref(img), cur.cuda_stream)
            return self._finished(binning, D, cap, shared, fp)
        with torch.cuda.device(a.means3D.device):
            self.d_ev.synchronize()
            d_host, fp_host = C.c_uint32(0), C.c_uint64(0)
            _lib.call(lib.texgs_num_rendered_reduce, pin.data_ptr(), a.N, C.byref(d_host), C.byref(fp_host))
            _pin_give(pin)
            D, fp = int(d_host.value), int(fp_host.value)
            shared = entry is not None and fp == entry.fingerprint and D == entry.D
            if shared:
                # same geometry as the forward that built `entry`: its lists are this forward's lists; K6 alone, no hand-off work
                _GEOM_STATS["hits"] += 1
                binning, cap = _lib.Binning(D, *entry.bin), entry.cap
                _lib.call(lib.texgs_render_forward, *refs, C.byref(binning), C.byref(img), stream)
                if for_backward and entry.handoff and (entry.counts or not self.want_counts):
                    img.survivors, img.surv_qmask, img.surv_count = entry.handoff
                    img.tex_bin_count, img.tex_bin_resv = entry.counts if self.want_counts else (None, None)
            else:
                _GEOM_STATS["misses"] += 1
                grown = int(D * 1.25) + 1024
                if entry is not None:       # expected to share, cannot: build the lists after all (K2 was not started before the sync)
                    cap = max(cap, grown)
                    self._alloc_bin(cap, None)
                    _lib.call(lib.texgs_depth_sort_scan, refs[2], a.N, stream)
                elif D > cap:               # rare: grow
                    cap = grown
                    self._alloc_bin(cap, self.fix)
                binning = self.binning
                binning.num_rendered = D
                _lib.call(lib.texgs_bin_sort_render_forward, *refs, C.byref(binning), C.byref(img), stream)
                _CAPACITY_HINT[self.hint_key] = max(_CAPACITY_HINT.get(self.hint_key, 0), grown)
                if GEOM_CACHE:
                    _GEOM[self.gkey] = _GeomEntry(          # (bin: every field of the binning after num_rendered)
                        self.gints, self.cam_key, fp, D, cap, tuple(getattr(binning, n) for n, _ in _lib.Binning._fields_[1:]),
                        (self.fix, self.bin_ar), (img.survivors, img.surv_qmask, img.surv_count) if self.handoff else None,
                        (img.tex_bin_count, img.tex_bin_resv) if (self.handoff and img.tex_bin_count) else None)
        return self._finished(binning, D, cap, shared, fp)

    def _finished(self, binning, D, cap, shared, fp):
        a, img, entry = self.args, self.img, self.entry
        for_backward, _, lazy = self.flags
        arenas = (self.fix,) + ((self.bin_ar,) if self.bin_ar is not None else ()) + (tuple(entry.arenas) if shared else ())
        # (NOT the output tensors: autograd hangs its node on them, the node holds this state -- a cycle that kept every dropped
        #  graph's buffers alive until the garbage collector ran)
        tensors = _Tensors(arenas, keep=self.keep, radii=self.outs[4], for_backward=bool(for_backward))
        for n in _HANDOFF:          # no hand-off in this state (forward-only call, lazy mode, or a shared entry without one)
            if getattr(img, n) is None:
                tensors[n] = None
        state = _State(self.frame, self.inputs, self.geom, binning, img, tensors, a, D, cap, self.tiles, self.want_counts,
                       bool(lazy and for_backward), shared)
        state.fingerprint = fp
        return self.outs, state

    def abandon(self):
        """A begun forward that will never be finished: its pinned block may go back to the pool only when the copy into it has landed."""
        if self.binned is not None:         # a view of a batched front end: its counts were read back there, nothing is in flight to the host
            return
        self.d_ev.synchronize()
        _pin_give(self.pin)


# ---- the batched front end: K1..K5 of the views of one multi-view step in one set of launches ------------------------------------
# Inside `with batched_prefetch():` prefetch_forward / GaussianRasterizer.prefetch only REGISTER their forward, with the stream they
# were called on.  On exit the requests are grouped: the same input tensors (storage, version, shape), image size, sh_degree, debug
# flag and for_backward / count_bins / lazy flags, on one device -- different cameras.  Every group of two or more runs K1..K5 once,
# on the stream current at the exit, through the entry points of include/texgs_multiview.h (_begin_views): K1 reads the SH rows once for
# all views, K2..K5 take the view as a grid dimension, ONE readback brings every view's instance count.  Each view is then left in
# _PREFETCH under the stream it was registered on, exactly as a prefetched forward that has begun, except that its forward has only K6
# left to run.  A request that fits no group (alone in its group, N == 0) takes today's path: begun at the exit, or -- begin_rest=False,
# which ViewPipeline.run uses to keep its one-view-per-stream-ahead rhythm for those -- left to the caller (request.batched is False).
# Groups of more than BATCH_MAX_VIEWS are cut into runs of that many.  The shared-geometry cache is bypassed for batched views.
_BATCH_SCOPE = None


class _Request:
    __slots__ = ("fwd", "stream", "batched")

    def __init__(self, fwd, stream):
        self.fwd, self.stream, self.batched = fwd, stream, False


def group_requests(keys, max_views, min_views=2):
    """Indices of `keys` -> (groups, rest): the runs of at most `max_views` requests with equal keys, in first-seen order, that hold at
    least `min_views` requests; `rest`: the indices left alone.  Pure (the grouping rule of batched_prefetch, testable without a device)."""
    by_key = {}
    for i, k in enumerate(keys):
        by_key.setdefault(k, []).append(i)
    groups, rest = [], []
    for idx in by_key.values():
        for lo in range(0, len(idx), max_views):
            run = idx[lo:lo + max_views]
            (groups if len(run) >= min_views else rest).append(run)
    return groups, sorted(i for run in rest for i in run)


def _batch_key(fwd):
    t = lambda x: None if x is None else (x.data_ptr(), x._version, tuple(x.shape), x.dtype, x.device)
    st = fwd.st
    return (int(st.image_height), int(st.image_width), int(st.sh_degree), bool(st.debug)) + tuple(t(x) for x in fwd.raw) + fwd.flags


class batched_prefetch:
    """Context manager: the forwards prefetched inside begin together at the exit (see above).  `requests`: what was registered, in
    order; nested scopes join the outermost one.  `min_views` (default 2; 1: a view alone goes through the batched entry points too, with
    one view in their tables -- nothing is gained, the kernels are the same; tests).

    The views of a scope are meant to be forwarded before the next scope closes: batched forwards of EARLIER scopes that are still parked
    then (their forward never came, or came with other tensors, versions or another stream) are dropped at that point -- each keeps its
    group's step buffers alive --, and such a forward simply runs per view if it is called after all."""

    def __init__(self, begin_rest=True, min_views=2):
        self.begin_rest, self.min_views, self.requests, self.outer = begin_rest, max(1, int(min_views)), [], None

    def __enter__(self):
        global _BATCH_SCOPE
        self.outer = _BATCH_SCOPE
        if self.outer is None:
            _BATCH_SCOPE = self
        else:
            self.requests = self.outer.requests
        return self

    def __exit__(self, exc_type, exc, tb):
        global _BATCH_SCOPE
        if self.outer is not None:
            return False
        _BATCH_SCOPE = None
        if exc_type is not None:
            return False            # nothing was launched for the registered forwards: they run when they are called
        from .multiview import BATCH_MAX_VIEWS
        reqs = self.requests
        groups, rest = group_requests([_batch_key(r.fwd) if r.fwd.raw[0].shape[0] > 0 else ("empty", i) for i, r in enumerate(reqs)],
                                      BATCH_MAX_VIEWS, self.min_views)
        if groups:
            _drop_parked_batched()
        for run in groups:
            _begin_views([reqs[i] for i in run])
        if self.begin_rest:
            for i in rest:
                with torch.cuda.stream(reqs[i].stream):
                    _register_begun(reqs[i].fwd.begin(), limit=4)
        return False


def _drop_parked_batched():
    """Batched forwards that no view picked up (batched_prefetch: dropped when the next scope batches): out of _PREFETCH, and with them
    the last references to their step buffers."""
    for key in list(_PREFETCH):
        lst = _PREFETCH[key] = [(k, f) for k, f in _PREFETCH[key] if f.binned is None]
        if not lst:
            del _PREFETCH[key]


def _register_begun(fwd, limit=None):
    device = fwd.args.means3D.device
    lst = _PREFETCH.setdefault((device.index, int(torch.cuda.current_stream(device).cuda_stream)), [])
    lst.append((fwd.key(), fwd))
    if limit is not None:
        for _, old in lst[:-limit]:
            old.abandon()
        del lst[:-limit]


def _begin_views(reqs):
    """K1..K5 of the forwards in `reqs` (one group of batched_prefetch, 2..BATCH_MAX_VIEWS views) on the current stream; every forward
    ends up in _PREFETCH under its own stream with its lists built."""
    from .multiview import views_entries
    lib, ent = _lib.load(), views_entries()
    fwds = [r.fwd for r in reqs]
    device = fwds[0].raw[0].device
    V = len(fwds)
    with torch.cuda.device(device):
        for f in fwds:
            f._plan(batched=True)
        a, N = fwds[0].args, fwds[0].args.N
        cur = torch.cuda.current_stream(device)
        others = {int(r.stream.cuda_stream): r.stream for r in reqs if r.stream.cuda_stream != cur.cuda_stream}

        def place(arenas, extra=0):
            """One step buffer for these arenas (+ `extra` bytes behind them) -> (buffer, offset of the extra bytes)"""
            offs, total = [], 0
            for ar in arenas:
                offs.append(total)
                total = (total + ar.size + 255) & ~255
            sb = _StepBuffer(total + extra, device)
            for s in others.values():           # used on the views' streams too: the allocator must not hand it out again before they are done
                sb.buf.record_stream(s)
            for ar, off in zip(arenas, offs):
                ar.place(sb, off)
            return sb, total

        words = int(lib.texgs_num_rendered_words(N))
        sb, sums_off = place([f.fix for f in fwds], extra=4 * V * words)
        sums = sb.buf[sums_off:sums_off + 4 * V * words].view(torch.int32)
        for f, r in zip(fwds, reqs):
            f._bind(batched=True)
            f.stream, f.cur_stream = int(cur.cuda_stream), cur          # (where this forward's K1..K5 run)
            if r.stream.cuda_stream != cur.cuda_stream:
                # made on this stream, used by K6..K8 on the view's: the outputs, and whatever _check_inputs / _make_frame had to copy
                # (an input or a camera tensor that was not contiguous f32) -- `keep` holds those beside the caller's own tensors
                for t in list(f.outs) + [t for t in f.keep if t is not None and t.is_cuda]:
                    t.record_stream(r.stream)
        frames = (_lib.Frame * V)(*[f.frame for f in fwds])
        geoms = (_lib.Geom * V)(*[f.geom for f in fwds])
        stream = cur.cuda_stream
        _lib.call(ent.preprocess_forward_views, frames, C.byref(fwds[0].inputs), geoms, V, sums.data_ptr(), stream)
        # ONE device->host read for all views; K2 of all views runs behind it while the host waits
        pin = _pin_take(V * words)
        pin.copy_(sums, non_blocking=True)
        d_ev = torch.cuda.Event()
        d_ev.record(cur)
        _lib.call(ent.depth_sort_scan_views, geoms, N, V, stream)
        d_ev.synchronize()
        counts = []
        d_host, fp_host = C.c_uint32(0), C.c_uint64(0)
        for v in range(V):
            _lib.call(lib.texgs_num_rendered_reduce, pin.data_ptr() + 4 * v * words, N, C.byref(d_host), C.byref(fp_host))
            counts.append((int(d_host.value), int(fp_host.value)))
        _pin_give(pin)
        # the arenas sized by the instance counts: exact per view (+ rounding), one allocation whose size follows the largest sum seen
        for f, (D, _) in zip(fwds, counts):
            f.cap = (max(D, 1) + 1023) & ~1023
            f._alloc_bin(f.cap, f.fix, commit=False)
        need = sum((f.bin_ar.size + 255) & ~255 for f in fwds)
        hint_key = ("views", device.index, N, fwds[0].gints[1], fwds[0].gints[2], V)
        hint = _CAPACITY_HINT.get(hint_key, 0)
        if need > hint:
            hint = _CAPACITY_HINT[hint_key] = need + need // 8
        place([f.bin_ar for f in fwds], extra=hint - need)
        for f, (D, _) in zip(fwds, counts):
            f._bind_bin(f.fix)
            f.binning.num_rendered = D
        bins = (_lib.Binning * V)(*[f.binning for f in fwds])
        imgs = (_lib.Image * V)(*[f.img for f in fwds])
        _lib.call(ent.bin_sort_views, frames, geoms, bins, imgs, V, stream)
        ready = torch.cuda.Event()
        ready.record(cur)
    for f, r, (D, fp) in zip(fwds, reqs, counts):
        f.binned, f.pin, r.batched = (D, fp, ready), None, True
        with torch.cuda.stream(r.stream):
            _register_begun(f)


def _gpu_only(device):
    _lib.load()
    if device.type != "cuda":
        raise RuntimeError("the textured rasterizer runs on an AMD GPU (torch device 'cuda' = HIP); "
                           f"got tensors on {device}. There is no CPU fallback.")


def prefetch_forward(st, means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset=None,
                     for_backward=True, cov3D_precomp=None, count_bins=None, lazy=False):
    """Begin a forward now -- K1, the asynchronous D readback, K2 -- on the current stream; a later forward_raw / GaussianRasterizer
    call on this stream with the same arguments (same tensor storages and versions, same settings, same flags) finishes it without
    waiting for the device.  At most four forwards are kept pending per stream (older ones are dropped: their K1 was wasted, and the
    host waits for it once).  Inside `with batched_prefetch():` the forward is only registered and begins when the scope closes, together
    with the other views registered there (K1..K5 once for all of them).  Returns nothing."""
    device = means3D.device
    _gpu_only(device)
    fwd = _Forward(st, (means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset, cov3D_precomp),
                   for_backward, count_bins, lazy)
    if _BATCH_SCOPE is not None:        # inside batched_prefetch: begun at its exit, together with the other views of the step
        _BATCH_SCOPE.requests.append(_Request(fwd, torch.cuda.current_stream(device)))
        return
    _register_begun(fwd.begin(), limit=4)


def forward_raw(st, means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset=None,
                for_backward=True, cov3D_precomp=None, count_bins=None, lazy=False):
    """Run K1..K6.  Returns (outputs, state).  No autograd here.

    `lazy` (the autograd path sets it): the hand-off may be left to the backward (the predictor above: unused_streak).

    `for_backward`: K6 leaves the per-block survivor lists its backward replays.  `count_bins` (default: for_backward and
    there is a texture): K6 also counts the texture-gradient footprints per texture bin (the exact list sizes of
    backward_raw's binned texture gradient); a caller that will not ask for dL/dtexture saves that work.
    `texture=None`: the untextured surface (diff_gauss, render/render.py:75-84): uvs / gradient_uvs may be None too.
    `cov3D_precomp` f32[N,6] (untextured surface only): used instead of scales / rotations."""
    _gpu_only(means3D.device)
    fwd = _Forward(st, (means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset, cov3D_precomp),
                   for_backward, count_bins, lazy)
    # was this very forward begun earlier (prefetch_forward)?  Then K1 ran long ago: finish that one
    pend = _prefetch_take(means3D.device, fwd.key()) if _PREFETCH else None
    return (pend or fwd.begin()).finish()


def _late_handoff(s: _State):
    """The forward left no survivor lists (lazy mode, or lists shared from a forward that had none): produce them now with one
    more K6 on the state's lists -- outputs into scratch (bit-identical to the forward's, which stay untouched)."""
    lib = _lib.load()
    device = s.args.means3D.device
    stream = torch.cuda.current_stream(device).cuda_stream
    ar = _Arena(device)
    _add_handoff(ar, s.cap, s.tiles, s.R, s.want_counts)
    ar.add("scratch_out", (8, s.H, s.W), torch.float32)
    ar.add("final_T", (s.H, s.W), torch.float32)
    ar.add("n_contrib", (s.H, s.W), torch.int32)
    ar.commit()
    so = ar.ptr("scratch_out")
    hw = 4 * s.H * s.W
    img = _lib.Image(so, so + 3 * hw, so + 4 * hw, so + 7 * hw, ar.ptr("final_T"), ar.ptr("n_contrib"), *(ar.ptr(n) for n in _HANDOFF))
    _lib.call(lib.texgs_render_forward, C.byref(s.frame), C.byref(s.inputs), C.byref(s.geom), C.byref(s.bin), C.byref(img), stream)
    s.tensors._arenas = tuple(s.tensors._arenas) + (ar,)
    for n in _HANDOFF:
        setattr(s.img, n, ar.ptr(n))
        s.tensors.pop(n, None)
        if n not in ar.specs:
            s.tensors[n] = None
    _GEOM_STATS["late_handoffs"] += 1


def _plan_outputs(N, K, textured, has_cov, has_coff, want, sinks, device):
    """Where K8 writes the per-Gaussian gradients -> (outs, mask, returned).  `outs`: name -> tensor, the sink where there is one, else
    a view of ONE fresh allocation; `mask`: the _ACC_BITS of the sinks (K8 adds into those); `returned`: what backward_raw hands back
    under each name (None for an output that went into a sink).  Nothing is planned without WANT_GAUSSIANS."""
    shapes = {}
    if want & _lib.WANT_GAUSSIANS:
        shapes = dict(means3D=(N, 3), means2D=(N, 3), opacities=(N, 1))
        if has_cov:
            shapes["cov3D"] = (N, 6)
        else:
            shapes.update(scales=(N, 3), rotations=(N, 4))
        if textured:
            shapes["uvs"] = (N, 3)
        if K > 0:
            shapes["shs"] = (N, K, 3)
        if has_coff:
            shapes["color_offset"] = (N, 3)
    fresh = [n for n in shapes if n not in sinks]
    sizes = [math.prod(shapes[n]) for n in fresh]
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=device).split(sizes) if fresh else ()
    outs, mask = {n: v.view(shapes[n]) for n, v in zip(fresh, flat)}, 0
    for n in shapes.keys() - set(fresh):
        t = outs[n] = sinks[n]
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == math.prod(shapes[n]), n
        mask |= _ACC_BITS[n]
    return outs, mask, {n: (None if n in sinks else outs[n]) for n in shapes}


def backward_raw(s: _State, dL_dcolor, dL_ddepth, dL_dnorm, dL_dalpha, sinks=None, before_accumulate=None,
                 want=_lib.WANT_ALL, defer_sh=None):
    """Run K7+K8.  Returns grads (means3D, means2D, shs, opacities, scales, rotations, uvs, texture).

    `want` (TEXGS_WANT_* bits): WANT_TEXTURE = dL/dtexture, WANT_GAUSSIANS = every per-Gaussian gradient.  What is not wanted
    is not computed (K7 is compiled in four flavours, K8 is skipped without WANT_GAUSSIANS) and comes back as None.

    `before_accumulate` (optional callable): invoked between K7 + bin reduce and K8 -- the point where a multi-view
    pipeline makes this stream wait for the previous view's K8 (texgs.multiview.ViewPipeline).

    `sinks` (optional): dict name -> existing float32 gradient buffer of the input's shape.  K8 ADDS into the sink of
    every per-Gaussian output that has one (TexGSGrads.accumulate bit mask: fused multi-view accumulation, or a leaf's
    existing .grad) and writes the others into one fresh allocation; a texture sink is used the same way (dL_dtexture is
    always accumulated into).  Outputs written into a sink come back as None.

    `defer_sh` (optional): (bucket, means3D leaf, shs leaf) -- a texgs.multiview.GradBucket in its deferred mode whose slices are
    the sinks of BOTH leaves.  K8 then leaves the view-dependent colour's chain to the bucket's flush: it gets a residue buffer from the bucket
    (TexGSGrads.dL_dvd_residue), which registers this view's camera position and degree with it."""
    lib = _lib.load()
    if not s.tensors["for_backward"]:
        raise RuntimeError("this forward ran with for_backward=False (no survivor lists were kept): its backward cannot run")
    a = s.args
    device = a.means3D.device
    f32 = dict(dtype=torch.float32, device=device)
    N, R = s.N, s.R
    stream = torch.cuda.current_stream(device).cuda_stream
    textured = a.texture is not None
    want &= _lib.WANT_ALL if textured else _lib.WANT_GAUSSIANS
    want_g, want_t = bool(want & _lib.WANT_GAUSSIANS), bool(want & _lib.WANT_TEXTURE)
    if not want:
        return (None,) * 8

    def g(t, shape):
        if t is None:
            return None
        t = t.to(torch.float32).contiguous()
        assert tuple(t.shape) == shape, (tuple(t.shape), shape)
        return t
    dc, dd, dn, da = g(dL_dcolor, (3, s.H, s.W)), g(dL_ddepth, (1, s.H, s.W)), g(dL_dnorm, (3, s.H, s.W)), g(dL_dalpha, (1, s.H, s.W))
    with torch.cuda.device(device):
        if s.img.survivors is None:
            _late_handoff(s)
        s.backward_ran = True
        if s.lazy:
            with _PRED_LOCK:
                _LAST_DIFFERENTIATED[device.index] = max(_LAST_DIFFERENTIATED.get(device.index, -1), s.serial)
        skey = (device.index, int(stream))
        sc = _SCRATCH.pop(skey, None) or SimpleNamespace(acc=None, bins=None)     # re-cached only after success (an exception drops it)
        if want_g and (sc.acc is None or sc.acc.shape[0] < max(N, 1)):
            sc.acc = torch.zeros(max(N, 1), _lib.ACC_FLOATS, **f32)
        acc = sc.acc if want_g else None
        sinks = sinks or {}
        outs, mask, res = _plan_outputs(N, s.K, textured, a.cov3D_precomp is not None, a.color_offset is not None, want, sinks, device)
        tex_sink = sinks.get("texture") if want_t else None
        d_tex = (tex_sink if tex_sink is not None else torch.zeros(6, R, R, 3, **f32)) if want_t else None
        bins = None
        if want_t and USE_TEX_BINS and s.tensors.get("tex_bin_count") is not None:
            bins = sc.bins if (sc.bins is not None and sc.bins.R == R) else _TexBins(lib, device, R)
            sc.bins = None
            bins.before_call(s.D, s.tensors.get("tex_bin_count"))
        grads = _lib.Grads(_ptr(dc), _ptr(dd), _ptr(dn), _ptr(da), _ptr(acc), _ptr(outs.get("means3D")), _ptr(outs.get("means2D")),
                           _ptr(outs.get("shs")), _ptr(outs.get("opacities")), _ptr(outs.get("scales")), _ptr(outs.get("rotations")),
                           _ptr(outs.get("uvs")), _ptr(d_tex), _ptr(outs.get("color_offset")), _ptr(outs.get("cov3D")), want,
                           _ptr(bins.rec) if bins else None, _ptr(bins.cursor) if bins else None,
                           _ptr(bins.base) if bins else None, bins.cap if bins else 0, mask, None)
        refs = [C.byref(x) for x in (s.frame, s.inputs, s.geom, s.bin, s.img, grads)]
        defer = defer_sh is not None and want_g and "shs" in outs and "means3D" in sinks and "shs" in sinks
        if before_accumulate is None and not defer:
            _lib.call(lib.texgs_backward, *refs, stream)
        else:
            _lib.call(lib.texgs_backward_render, *refs, stream)
            if before_accumulate is not None:
                before_accumulate()
            if defer:
                # (here, not earlier: after before_accumulate this stream is ordered behind every earlier view's K8, which is what an
                #  early flush of a full pool -- it reads their residues and adds into the sinks -- needs)
                bucket, leaf_m, leaf_s = defer_sh
                if bucket.deferred_pool_full(a.means3D):
                    bucket.flush_pending()
                campos = s.tensors["keep"][-1]           # (_make_frame appends bg, viewmatrix, projmatrix, campos last)
                assert campos.data_ptr() == s.frame.campos
                residue = bucket.sh_residue_for(leaf_m, leaf_s, a.means3D, a.shs, campos, s.frame.sh_degree)
                grads.dL_dvd_residue = residue.data_ptr()
            _lib.call(lib.texgs_backward_preprocess, *refs[:3], refs[5], stream)
    if bins is not None:
        bins.after_call()
        sc.bins = bins
    _SCRATCH[skey] = sc
    s.tensors["d_color_offset"] = res.get("color_offset")
    s.tensors["d_cov3D"] = res.get("cov3D")
    return tuple(res.get(n) for n in ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "uvs")) \
        + (None if tex_sink is not None else d_tex,)


def _leaf_grad_sink(t):
    """A leaf's existing, contiguous float32 .grad of the right shape (the kernels then add into it directly: no zero-filled
    temporary, no AccumulateGrad pass), else None."""
    if t is None or not (t.is_leaf and t.requires_grad):
        return None
    if getattr(t, "_backward_hooks", None) or getattr(t, "_post_accumulate_grad_hooks", None):
        return None             # a hook must see the gradient: let autograd deliver it
    gr = t.grad
    if gr is None or gr.dtype != torch.float32 or not gr.is_contiguous() or gr.shape != t.shape or gr.device != t.device:
        return None
    return gr


# inputs of _RasterizeGaussians.apply by position; the per-Gaussian ones decide TEXGS_WANT_GAUSSIANS
_ARG = dict(means3D=0, means2D=1, shs=2, opacities=3, scales=4, rotations=5, uvs=6, gradient_uvs=7, texture=8, st=9,
            color_offset=10, grad_sink=11, cov3D_precomp=12)
_GAUSSIAN_ARGS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "uvs", "color_offset", "cov3D_precomp")


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, st, color_offset=None,
                grad_sink=None, cov3D_precomp=None):
        ctx.grad_sink = grad_sink
        ctx.set_materialize_grads(False)     # outputs without an upstream gradient arrive as None, not as zero-filled tensors
        # the inputs by name: the backward looks at them again (bucket slices / leaf .grad buffers to accumulate into)
        ctx.named = dict(means3D=means3D, means2D=means2D, shs=shs, opacities=opacities, scales=scales,
                         rotations=rotations, uvs=uvs, texture=texture, color_offset=color_offset, cov3D=cov3D_precomp)
        # what the backward will be asked for decides what the forward prepares and what the backward computes: the texture
        # gradient (K6's per-bin footprint counts, K7's records, the bin reduce) only if the texture wants one; the per-Gaussian
        # stages (K7's recurrence + moment sums, K8) only if some per-Gaussian input does (texgs.h TEXGS_WANT_*)
        nig = tuple(ctx.needs_input_grad) + (False,) * len(_ARG)      # (apply() may be called without the trailing optional inputs)
        want = (_lib.WANT_TEXTURE if (texture is not None and nig[_ARG["texture"]]) else 0) \
            | (_lib.WANT_GAUSSIANS if any(nig[_ARG[n]] for n in _GAUSSIAN_ARGS) else 0)
        ctx.want = want
        ctx.nargs = len(ctx.needs_input_grad)
        # (autograd does not record inside Function.forward: the inputs go in as they are, no detach() copies of the tensor objects)
        outs, state = forward_raw(st, means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, color_offset,
                                  for_backward=bool(want), cov3D_precomp=cov3D_precomp,
                                  count_bins=bool(want & _lib.WANT_TEXTURE), lazy=True)
        color, depth, norm, alpha, radii = outs
        ctx.state = state
        # the backward re-reads the inputs through raw pointers (K8 recomputes geometry, K7 re-fetches texels): remember
        # their autograd version counters so an in-place update in between (optimizer.step, change_texture) is an error,
        # not a silently wrong gradient
        ctx.versions = [(t, t._version) for t in state.tensors["keep"] if t is not None]
        ctx.op_shape = opacities.shape
        ctx.mark_non_differentiable(radii)
        return color, depth, norm, alpha, radii

    @staticmethod
    def backward(ctx, dL_dcolor, dL_ddepth, dL_dnorm, dL_dalpha, _dradii):
        s = ctx.state
        if s is None:
            raise RuntimeError("the rasterizer's backward ran a second time: its per-call state was released after the "
                               "first backward (retain_graph=True is not supported); run the forward again")
        for t, v in ctx.versions:
            if t._version != v:
                raise RuntimeError("an input of the rasterizer was modified in place between its forward and backward "
                                   "(the backward re-reads inputs through saved pointers); clone it before modifying")
        # where the gradients go: (1) the slices of a texgs.multiview.GradBucket (fused multi-view accumulation) when one is
        # attached; (2) opt-in (TEXGS_DIRECT_LEAF_GRADS=1), for an input that is a hook-free LEAF whose .grad already exists,
        # that .grad itself; (3) fresh tensors handed back to autograd for everything else (the default).
        sinks, bucket = {}, False
        if ctx.grad_sink is not None:
            sinks = {k: g for k, g in ((k, ctx.grad_sink.sink_for(v)) for k, v in ctx.named.items() if v is not None)
                     if g is not None}
            bucket = bool(sinks)
        if not bucket and DIRECT_LEAF_GRADS:
            sinks = {k: g for k, g in ((k, _leaf_grad_sink(v)) for k, v in ctx.named.items()) if g is not None}
        wants_deferred = getattr(ctx.grad_sink, "wants_deferred", None) if bucket else None
        defer = wants_deferred is not None and wants_deferred(ctx.named["means3D"], ctx.named["shs"])
        d_means3D, d_means2D, d_shs, d_op, d_scales, d_rot, d_uvs, d_tex = backward_raw(
            s, dL_dcolor, dL_ddepth, dL_dnorm, dL_dalpha, sinks=sinks or None,
            before_accumulate=getattr(ctx.grad_sink, "before_accumulate", None) if bucket else None, want=ctx.want,
            defer_sh=(ctx.grad_sink, ctx.named["means3D"], ctx.named["shs"]) if defer else None)
        d_coff = s.tensors.get("d_color_offset")
        d_cov = s.tensors.get("d_cov3D")
        ctx.state = None
        ctx.versions = None
        ctx.named = None
        if d_op is not None:
            d_op = d_op.reshape(ctx.op_shape)
        return (d_means3D, d_means2D, d_shs, d_op, d_scales, d_rot, d_uvs, None, d_tex, None, d_coff, None, d_cov)[:ctx.nargs]


EXTRA_ATTRS_MAX = 32


def blend_extra_attrs(st, means3D, means2D, opacities, scales, rotations, extra_attrs, grad_sink=None, cov3D_precomp=None):
    """extra[C,H,W] = sum_i w_i * extra_attrs[i, c]: the lineage operator's `extra_attrs` kwarg / sixth return value
    (render/uv_tex_render.py:66,76, render/render.py:84 -- the reference itself always passes None).  Blended like depth and normals:
    no background term, no clamp.  NOT a fused path: ceil(C / 3) more passes of the UNTEXTURED operator (K1 + K6 on the lists of the
    main pass -- same camera, same Gaussians: the shared-geometry path -- and its own backward), three channels at a time as the
    pass's colour.  The colour path clamps at zero, so the attributes go in shifted by m = min(extra_attrs) - 1 (> 0 everywhere: the
    clamp never acts, its gradient mask never bites) and m * alpha is added back.  Differentiable w.r.t. extra_attrs and every
    geometry input through plain autograd."""
    N = means3D.shape[0]
    if not isinstance(extra_attrs, torch.Tensor) or extra_attrs.dim() != 2 or extra_attrs.shape[0] != N:
        raise ValueError(f"extra_attrs must be a [N, C] tensor with N = {N} rows")
    C_ = int(extra_attrs.shape[1])
    if C_ > EXTRA_ATTRS_MAX:
        raise ValueError(f"extra_attrs has {C_} channels; at most {EXTRA_ATTRS_MAX} are blended")
    H, W = int(st.image_height), int(st.image_width)
    ea = extra_attrs.to(torch.float32)
    if C_ == 0 or N == 0:
        return torch.zeros(C_, H, W, dtype=torch.float32, device=means3D.device) + 0.0 * ea.sum()
    m = ea.detach().amin() - 1.0                       # (a device scalar: no sync)
    st0 = st._replace(bg=torch.zeros_like(st.bg), sh_degree=0)
    if means2D is None:
        means2D = torch.zeros_like(means3D)
    outs = []
    for c0 in range(0, C_, 3):
        grp = ea[:, c0:c0 + 3]
        if grp.shape[1] < 3:
            grp = torch.cat([grp, (m + 1.0).expand(N, 3 - grp.shape[1])], dim=1)
        color, _, _, alpha, _ = _RasterizeGaussians.apply(means3D, means2D, None, opacities, scales, rotations, None, None, None, st0,
                                                          ((grp - m) - 0.5).contiguous(), grad_sink, cov3D_precomp)
        outs.append(color + m * alpha)
    return torch.cat(outs, dim=0)[:C_]


class GaussianRasterizer(nn.Module):
    """Same call surface as the reference's rasterizer (render/uv_tex_render.py:40,56-66)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings, grad_sink=None):
        super().__init__()
        self.raster_settings = raster_settings
        # optional texgs.multiview.GradBucket: gradients of inputs that are its registered leaves are accumulated
        # into the bucket by the kernels themselves (no autograd AccumulateGrad pass); not part of the reference API
        self.grad_sink = grad_sink

    def markVisible(self, positions):
        """Frustum test only (lineage API; unused by the reference)."""
        lib = _lib.load()
        st = self.raster_settings
        positions = _f32c(positions, "positions", positions.device)
        N = positions.shape[0]
        keep = []
        frame = _make_frame(st, N, 0, 1, positions.device, keep)
        vis = torch.zeros(N, dtype=torch.uint8, device=positions.device)
        stream = torch.cuda.current_stream(positions.device).cuda_stream
        with torch.cuda.device(positions.device):
            _lib.call(lib.texgs_mark_visible, C.byref(frame), positions.data_ptr(), vis.data_ptr(), stream)
        return vis.bool()

    def prefetch(self, means3D, means2D, opacities, shs=None, scales=None, rotations=None, uvs=None,
                 gradient_uvs=None, texture=None, extra_attrs=None):
        """Begin this forward now (K1 + the asynchronous instance-count readback + K2, on the current stream); the same call through
        forward() later -- same tensors, unchanged in between, same settings tensors, same stream -- finishes it without waiting for
        whatever the stream was given in the meantime (prefetch_forward).  Not part of the reference API; a no-op for its results."""
        grad = torch.is_grad_enabled()
        rg = lambda t: bool(grad and t is not None and t.requires_grad)
        want_tex = rg(texture)
        want_g = any(rg(t) for t in (means3D, means2D, shs, opacities, scales, rotations, uvs))
        prefetch_forward(self.raster_settings, means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, None,
                         for_backward=want_tex or want_g, cov3D_precomp=None, count_bins=want_tex, lazy=True)

    def forward(self, means3D, means2D, opacities, shs=None, scales=None, rotations=None, uvs=None,
                gradient_uvs=None, texture=None, extra_attrs=None):
        st = self.raster_settings
        if scales is None or rotations is None:
            raise ValueError("scales and rotations are required (the textured operator has no cov3D_precomp path)")
        if uvs is None or gradient_uvs is None or texture is None:
            raise ValueError("uvs, gradient_uvs and texture are required")
        if means2D is None:
            means2D = torch.zeros_like(means3D)
        color, depth, norm, alpha, radii = _RasterizeGaussians.apply(
            means3D, means2D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture, st, None, self.grad_sink)
        extra = None
        if extra_attrs is not None:         # (always None in the reference, render/uv_tex_render.py:66; see blend_extra_attrs)
            extra = blend_extra_attrs(st, means3D, means2D, opacities, scales, rotations, extra_attrs, self.grad_sink)
        return color, depth, norm, alpha, radii, extra
