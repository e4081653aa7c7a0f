"""The rasterizer's host layer without a GPU: input validation, the arena, the K6 -> K7 hand-off layout and the backward's output
plan are plain Python over torch tensors, so they run on CPU tensors (texgs/rasterizer.py _check_inputs, _Arena, _add_handoff,
_plan_outputs)."""
import math

import pytest
import torch

from texgs import _lib
from texgs import rasterizer as RZ


def _settings(sh_degree=3):
    z = torch.zeros
    return RZ.GaussianRasterizationSettings(40, 72, 0.5, 0.5, z(3), 1.0, z(4, 4), z(4, 4), sh_degree, z(3), False, False)


def _inputs(N, R=4, K=3):
    """means3D, shs, opacities, scales, rotations, uvs, gradient_uvs, texture: a valid textured call."""
    z = torch.zeros
    return dict(means3D=z(N, 3), shs=z(N, K, 3), opacities=z(N, 1), scales=z(N, 3), rotations=z(N, 4), uvs=z(N, 3),
                gradient_uvs=z(N, 3, 3), texture=z(6, R, R, 3))


@pytest.mark.parametrize("N", [0, 5])
def test_check_inputs_accepts_a_valid_call(N):
    a = RZ._check_inputs(_settings(), **_inputs(N, R=4, K=3))
    assert (a.N, a.K, a.R) == (N, 3, 4)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in a[:8])
    assert a.color_offset is None and a.cov3D_precomp is None
    # the untextured surface: no texture, no uvs, a precomputed covariance instead of scales / rotations
    kw = dict(_inputs(N), uvs=None, gradient_uvs=None, texture=None, shs=None, scales=None, rotations=None)
    a = RZ._check_inputs(_settings(), **kw, color_offset=torch.zeros(N, 3), cov3D_precomp=torch.zeros(N, 6))
    assert (a.N, a.K, a.R) == (N, 0, 1)
    assert a.scales is None and a.rotations is None and a.uvs is None and a.gradient_uvs is None and a.texture is None
    assert a.cov3D_precomp.shape == (N, 6) and a.color_offset.shape == (N, 3)


_N = 5
_REJECTED = [
    ("means3D rank", dict(means3D=torch.zeros(_N)), ValueError),
    ("opacities rows", dict(opacities=torch.zeros(_N + 1, 1)), ValueError),
    ("scales rows", dict(scales=torch.zeros(_N + 1, 3)), ValueError),
    ("rotations rows", dict(rotations=torch.zeros(_N - 1, 4)), ValueError),
    ("uvs rows", dict(uvs=torch.zeros(_N + 1, 3)), ValueError),
    ("gradient_uvs numel", dict(gradient_uvs=torch.zeros(_N, 3, 2)), ValueError),
    ("texture not [6,R,R,3]", dict(texture=torch.zeros(6, 4, 5, 3)), ValueError),
    ("texture faces", dict(texture=torch.zeros(5, 4, 4, 3)), ValueError),
    ("shs K = 16", dict(shs=torch.zeros(_N, 16, 3)), ValueError),
    ("color_offset shape", dict(color_offset=torch.zeros(_N, 4)), ValueError),
    ("cov3D_precomp with a texture", dict(cov3D_precomp=torch.zeros(_N, 6)), ValueError),
    ("float64 means3D", dict(means3D=torch.zeros(_N, 3, dtype=torch.float64)), TypeError),
    ("float16 texture", dict(texture=torch.zeros(6, 4, 4, 3, dtype=torch.float16)), TypeError),
    ("not a tensor", dict(opacities=[0.0] * _N), TypeError),
]


@pytest.mark.parametrize("what,change,exc", _REJECTED, ids=[r[0] for r in _REJECTED])
def test_check_inputs_rejects(what, change, exc):
    with pytest.raises(exc):
        RZ._check_inputs(_settings(), **dict(_inputs(_N), **change))


def test_check_inputs_rejects_sh_degree_out_of_range():
    with pytest.raises(ValueError):
        RZ._check_inputs(_settings(sh_degree=4), **_inputs(_N))


def test_arena_on_the_cpu_device():
    ar = RZ._Arena(torch.device("cpu"))
    decl = dict(a=((3, 5), torch.float32), b=((7,), torch.int16), c=((1,), torch.uint8), d=((2, 3, 2), torch.int64), e=((0,), torch.int32),
                f=((129,), torch.int32))
    for n, (shape, dt) in decl.items():
        ar.add(n, shape, dt)
    ar.commit()
    spans = []
    for n, (shape, dt) in decl.items():
        off = ar.specs[n][0]
        assert off % 256 == 0
        v = ar.view(n)
        assert tuple(v.shape) == shape and v.dtype == dt
        assert ar.ptr(n) == ar.buf.data_ptr() + off and (v.numel() == 0 or v.data_ptr() == ar.ptr(n))
        spans.append((off, off + math.prod(shape) * dt.itemsize))
    spans.sort()
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))          # disjoint
    assert spans[-1][1] <= ar.buf.numel()
    assert ar.ptr("absent") is None


def _handoff_specs(*arenas):
    return {n: ar.specs[n][1:] for ar in arenas for n in ar.specs if n in RZ._HANDOFF}


@pytest.mark.parametrize("cap,tiles,R,want_counts", [(0, 1, 1, False), (7, 6, 33, True)])
def test_handoff_layout_is_the_same_for_the_forward_and_the_late_handoff(lib_built, cap, tiles, R, want_counts):
    lib, cpu = _lib.load(), torch.device("cpu")
    i32, c = torch.int32, 4 * max(cap, 1)
    expect = {"survivors": ((c, 2), i32), "surv_qmask": ((c,), torch.int16), "surv_count": ((4 * tiles,), i32)}
    if want_counts:
        expect["tex_bin_count"] = ((2 * int(lib.texgs_tex_bin_count(R)),), i32)
        expect["tex_bin_resv"] = ((4 * tiles, _lib.RESV_WORDS), i32)
    # the eager path, as an ordinary forward allocates: per-tile pieces in the fixed arena, the D-sized ones in the bin arena ...
    f = RZ._Forward.__new__(RZ._Forward)
    f.tiles, f.handoff, f.want_counts, f.img = tiles, True, want_counts, _lib.Image()
    f.args = RZ._check_inputs(_settings(), **_inputs(2, R=R))
    f.fix = RZ._Arena(cpu)
    f._add_lists(f.fix)
    f.fix.commit()
    f._alloc_bin(cap, f.fix)
    assert _handoff_specs(f.fix, f.bin_ar) == expect
    assert {"survivors", "surv_qmask"} <= set(f.bin_ar.specs) and "surv_count" in f.fix.specs and "ranges" in f.fix.specs
    for n in RZ._HANDOFF:
        assert getattr(f.img, n) == (f.bin_ar.ptr(n) or f.fix.ptr(n))
    # ... as a candidate that has to build lists after all allocates: everything in the bin arena ...
    f.fix, f.img = RZ._Arena(cpu), _lib.Image()
    f._alloc_bin(cap, None)
    assert _handoff_specs(f.bin_ar) == expect and "ranges" in f.bin_ar.specs
    for n in RZ._HANDOFF:
        assert getattr(f.img, n) == f.bin_ar.ptr(n)
    # ... and the backward's late hand-off: one arena
    late = RZ._Arena(cpu)
    RZ._add_handoff(late, cap, tiles, R, want_counts)
    assert _handoff_specs(late) == expect and set(late.specs) == set(expect)
    # a forward without a hand-off (forward-only call, lazy mode) allocates none of it
    f.handoff, f.fix, f.img = False, RZ._Arena(cpu), _lib.Image()
    f._alloc_bin(cap, None)
    assert _handoff_specs(f.bin_ar) == {} and all(getattr(f.img, n) is None for n in RZ._HANDOFF)


_PLANS = [
    ("untextured_cov", dict(N=6, K=2, textured=False, has_cov=True, has_coff=False),
     dict(means3D=(6, 3), means2D=(6, 3), opacities=(6, 1), cov3D=(6, 6), shs=(6, 2, 3))),
    ("textured_K3_coff", dict(N=5, K=3, textured=True, has_cov=False, has_coff=True),
     dict(means3D=(5, 3), means2D=(5, 3), opacities=(5, 1), scales=(5, 3), rotations=(5, 4), uvs=(5, 3), shs=(5, 3, 3),
          color_offset=(5, 3))),
]


@pytest.mark.parametrize("name,kw,shapes", _PLANS, ids=[p[0] for p in _PLANS])
@pytest.mark.parametrize("sink_names", [(), ("means3D", "shs")], ids=["no_sinks", "sinks"])
def test_plan_outputs(name, kw, shapes, sink_names):
    cpu = torch.device("cpu")
    sinks = {n: torch.zeros(shapes[n]) for n in sink_names}
    outs, mask, returned = RZ._plan_outputs(kw["N"], kw["K"], kw["textured"], kw["has_cov"], kw["has_coff"], _lib.WANT_ALL, sinks, cpu)
    assert {n: tuple(t.shape) for n, t in outs.items()} == shapes and set(returned) == set(shapes)
    assert mask == sum(RZ._ACC_BITS[n] for n in sink_names)
    fresh = [n for n in shapes if n not in sink_names]
    for n in sink_names:
        assert outs[n] is sinks[n] and returned[n] is None
    for n in fresh:
        assert returned[n] is outs[n] and outs[n].dtype == torch.float32 and outs[n].is_contiguous()
    store = {outs[n].untyped_storage().data_ptr() for n in fresh}
    assert len(store) == 1                                                   # one allocation ...
    assert outs[fresh[0]].untyped_storage().nbytes() == 4 * sum(math.prod(shapes[n]) for n in fresh)     # ... of exactly their sizes ...
    spans = sorted((outs[n].data_ptr(), outs[n].data_ptr() + 4 * outs[n].numel()) for n in fresh)
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))        # ... in which they do not overlap
    assert all(outs[n].untyped_storage().data_ptr() not in store for n in sink_names)
    # the texture gradient alone: no per-Gaussian output at all, whatever the sinks
    assert RZ._plan_outputs(kw["N"], kw["K"], kw["textured"], kw["has_cov"], kw["has_coff"], _lib.WANT_TEXTURE, sinks, cpu) == ({}, 0, {})
