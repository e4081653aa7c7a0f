"""Stage-1 density control of Texture-GS without its boolean-mask indexing (csrc/density.hip): what models/gaussian3d.py:200-350 and
the densification lines of optimize_step (:424-462) do to the NUMBER of Gaussians.

* `add_densification_stats`: the three masked updates of every stage-1 step (:431-432, :334-336) in one launch, nothing read back.
* `densify_and_prune` (:318-332): one classification of the N0 Gaussians the call starts from, three plain scan launches, ONE readback
  of four totals (the call's only synchronisation), then one launch that writes every row of the six parameters and their Adam moments
  exactly once.  The reference re-materialises all of them four times (cat, cat, mask, mask).
* `opacity_prune` (:338-341): the same machinery with nothing cloned or split.
* `reset_opacity` (:180-183), `reset_min_scale` (:343-350): plain element-wise torch on the device, no synchronisation.

The optimizer stays `torch.optim.Adam`: one parameter per group, every group carries a "name"; its state is edited the way the
reference edits it (`exp_avg` / `exp_avg_sq` replaced, `step` untouched, a group without state stays without).  Output rows: the
surviving originals in index order, the surviving clones, the surviving first children, the surviving second children.

Two things differ from a literal reading of the reference, both on purpose:
* `max_screen_size` only SWITCHES the world-size prune (`max scale > 0.1 extent`) on.  Its own term, `max_radii2D > max_screen_size`,
  can never fire there: densification_postfix zeroes max_radii2D for every row (:274-276) before densify_and_prune reads it (:327).
  The argument is kept and the reference followed.
* torch.normal's random stream is not reproduced.  The standard-normal samples of the split are an INPUT (`noise f32[2 ns, 3]`, row
  c ns + j for child c of the j-th split parent in index order, parents whose children are pruned included); without it they are drawn
  with torch.randn on the device.  A child's position is xyz + R(q/|q|) (s * eps), which is what normal(0, s) rotated is.

No CPU fallback: CPU tensors raise.  The C entry points take bare pointers, so every argument is checked here, before any launch.
No empty_cache() anywhere.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_KIND = {"xyz": "xyz", "scaling": "scaling"}
_WIDTH = {"xyz": 3, "f_dc": 3, "opacity": 1, "scaling": 3, "rotation": 4}


class DensityState:
    """The three running statistics of stage 1: xyz_gradient_accum f32[N, 1], denom f32[N, 1], max_radii2D f32[N]."""

    def __init__(self, xyz_gradient_accum, denom, max_radii2D):
        self.xyz_gradient_accum, self.denom, self.max_radii2D = xyz_gradient_accum, denom, max_radii2D

    @classmethod
    def zeros(cls, n, device):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        return cls(z(n, 1), z(n, 1), z(n))

    @property
    def N(self):
        return self.max_radii2D.shape[0]


def _need(t, what, shape, dtype, n=None, seen=None):
    """t is a contiguous tensor of that dtype and shape (None in `shape` = the row count, which must be `n` when given).  That it is
    on the GPU is checked at once, or -- with a list `seen` -- by _on_gpu(seen) after every shape of the call has been checked."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    ok = t.dim() == len(shape) and all(want is None or have == want for have, want in zip(t.shape, shape))
    if not ok:
        raise ValueError(f"{what} must be [{', '.join('N' if s is None else str(s) for s in shape)}], got {tuple(t.shape)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{what} holds {t.shape[0]} rows, the other arguments {n}")
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{what} holds {t.shape[0]} rows; the library indexes them with 32 bits")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if seen is None:
        _on_gpu([(t, what)])
    else:
        seen.append((t, what))
    return t


def _on_gpu(seen):
    for t, what in seen:
        if t.device.type != "cuda":
            raise RuntimeError(f"{what} must be on an AMD GPU; there is no CPU fallback")
    if len({t.device for t, _ in seen}) > 1:
        raise ValueError(f"{seen[0][1].split(':')[0]}: the tensors are on different devices")


def _check_state(state, what, n=None, seen=None):
    if not all(hasattr(state, k) for k in ("xyz_gradient_accum", "denom", "max_radii2D")):
        raise TypeError(f"{what}: state must hold xyz_gradient_accum, denom and max_radii2D (texgs.density.DensityState)")
    late = [] if seen is None else seen
    _need(state.max_radii2D, f"{what}: state.max_radii2D", (None,), torch.float32, n, late)
    n = state.max_radii2D.shape[0]
    _need(state.xyz_gradient_accum, f"{what}: state.xyz_gradient_accum", (None, 1), torch.float32, n, late)
    _need(state.denom, f"{what}: state.denom", (None, 1), torch.float32, n, late)
    if seen is None:
        _on_gpu(late)
    return n


def add_densification_stats(state, viewspace_grad, radii):
    """For every i with radii[i] > 0 (the reference's visibility filter): accum += sqrt(gx*gx + gy*gy) in fp32 without FMA,
    denom += 1, max_radii2D = max(max_radii2D, radii).  `state` is updated in place; one kernel on the current stream.
    viewspace_grad f32[N, 3] (the grad of the means2D carrier), radii int32[N] (as the rasterizers return it)."""
    what = "add_densification_stats"
    seen = []
    n = _check_state(state, what, None, seen)
    _need(viewspace_grad, f"{what}: viewspace_grad", (None, 3), torch.float32, n, seen)
    _need(radii, f"{what}: radii", (None,), torch.int32, n, seen)
    _on_gpu(seen)
    dev = state.max_radii2D.device
    lib = _lib.load()
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_density_stats, viewspace_grad.data_ptr(), radii.data_ptr(), n, state.xyz_gradient_accum.data_ptr(),
                  state.denom.data_ptr(), state.max_radii2D.data_ptr(), stream)


def _groups(params, optimizer, what, seen):
    """-> ({name: group}, {name: detached contiguous parameter data}, N) after every check of the parameter set"""
    if not isinstance(params, dict):
        raise TypeError(f"{what}: params must be a dict of the parameters by group name, got {type(params).__name__}")
    if not isinstance(optimizer, torch.optim.Optimizer):
        raise TypeError(f"{what}: optimizer must be a torch.optim.Optimizer, got {type(optimizer).__name__}")
    by_name = {}
    for g in optimizer.param_groups:
        if "name" not in g:
            raise ValueError(f"{what}: every param group of the optimizer needs a \"name\"")
        if len(g["params"]) != 1:
            raise ValueError(f"{what}: group {g['name']!r} holds {len(g['params'])} parameters, expected one")
        by_name[g["name"]] = g
    for name in GROUPS:
        if name not in params:
            raise KeyError(f"{what}: params lacks the group {name!r}")
        if name not in by_name:
            raise KeyError(f"{what}: the optimizer has no group named {name!r}")
    extra = sorted(set(by_name) - set(GROUPS))
    if extra:
        raise ValueError(f"{what}: the optimizer has groups this module does not resize: {', '.join(extra)}")
    n = params["xyz"].shape[0] if isinstance(params["xyz"], torch.Tensor) and params["xyz"].dim() >= 1 else None
    data = {}
    for name in GROUPS:
        p = params[name]
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"{what}: params[{name!r}] must be a torch.Tensor, got {type(p).__name__}")
        if p is not by_name[name]["params"][0]:
            raise ValueError(f"{what}: params[{name!r}] is not the parameter the optimizer holds for that group")
        if name in _WIDTH:
            shape = (None, 1, 3) if name == "f_dc" and p.dim() == 3 else (None, _WIDTH[name])
        else:
            shape = (None, None, 3) if p.dim() == 3 else (None, None)
        _need(p, f"{what}: params[{name!r}]", shape, torch.float32, n, seen)
        data[name] = p.detach()
    for name in GROUPS:
        st = optimizer.state.get(by_name[name]["params"][0])
        if st:
            for k in ("exp_avg", "exp_avg_sq"):
                if k not in st:
                    raise ValueError(f"{what}: the optimizer state of {name!r} has no {k} (torch.optim.Adam expected)")
                _need(st[k], f"{what}: {k} of {name!r}", tuple(None if i == 0 else s for i, s in enumerate(data[name].shape)),
                      torch.float32, n, seen)
    return by_name, data, n


def _number(x, what):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise TypeError(f"{what} must be a number, got {type(x).__name__}")
    return float(x)


def _plan(lib, data, state, n, dev, stream, max_grad, min_opacity, dense_scale, big_scale, densify, use_big):
    action = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    rank = torch.empty((4, max(n, 1)), dtype=torch.int32, device=dev)
    totals = torch.empty(4, dtype=torch.int32, device=dev)
    temp = torch.empty(lib.texgs_density_plan_temp_bytes(n), dtype=torch.uint8, device=dev)
    plan = _lib.DensityPlanStruct(state.xyz_gradient_accum.data_ptr() if densify else None, state.denom.data_ptr() if densify else None,
                                  data["scaling"].data_ptr(), data["opacity"].data_ptr(), n, max_grad, min_opacity, dense_scale,
                                  big_scale, int(densify), int(use_big))
    _lib.call(lib.texgs_density_plan, C.byref(plan), action.data_ptr(), rank.data_ptr(), totals.data_ptr(), temp.data_ptr(), stream)
    return action, rank, totals


def _plan_densify(params_data, state, *, max_grad, min_opacity, dense_scale, big_scale, densify=True, use_big=True):
    """The plan alone -- not part of the public interface: tests/test_density_gpu.py and scripts/bench_density.py compare it with the
    numpy statement.  (action u8[N], rank i32[4, N], totals i32[4]) of texgs_density_plan for the raw `scaling` f32[N, 3] and
    `opacity` f32[N, 1] in `params_data` and the state's accum / denom; arguments checked like the public calls'."""
    what = "_plan_densify"
    if not isinstance(params_data, dict):
        raise TypeError(f"{what}: params_data must be a dict, got {type(params_data).__name__}")
    for name in ("scaling", "opacity"):
        if name not in params_data:
            raise KeyError(f"{what}: params_data lacks {name!r}")
    max_grad, min_opacity = _number(max_grad, f"{what}: max_grad"), _number(min_opacity, f"{what}: min_opacity")
    dense_scale, big_scale = _number(dense_scale, f"{what}: dense_scale"), _number(big_scale, f"{what}: big_scale")
    if densify and not max_grad > 0:
        raise ValueError(f"{what}: max_grad must be positive, got {max_grad}")
    seen = []
    n = _check_state(state, what, None, seen)
    _need(params_data["scaling"], f"{what}: scaling", (None, 3), torch.float32, n, seen)
    _need(params_data["opacity"], f"{what}: opacity", (None, 1), torch.float32, n, seen)
    _on_gpu(seen)
    dev = state.max_radii2D.device
    lib = _lib.load()
    with _lib.on(dev) as stream:
        action, rank, totals = _plan(lib, params_data, state, n, dev, stream, max_grad, min_opacity, dense_scale, big_scale, bool(densify),
                                     bool(use_big))
    return action[:n], rank[:, :n], totals


def _resize(what, params, optimizer, state, max_grad, min_opacity, dense_scale, big_scale, densify, use_big, noise, generator,
            keep_state=False):
    seen = []
    by_name, data, n = _groups(params, optimizer, what, seen)
    _check_state(state, what, n, seen)
    if noise is not None:
        _need(noise, f"{what}: noise", (None, 3), torch.float32, None, seen)
    _on_gpu(seen)
    dev = data["xyz"].device
    lib = _lib.load()
    with _lib.on(dev) as stream:
        action, rank, totals = _plan(lib, data, state, n, dev, stream, max_grad, min_opacity, dense_scale, big_scale, densify, use_big)
        n_kept, n_clone, n_split, n_child = (int(v) for v in totals.tolist())        # the call's one synchronisation
        m = n_kept + n_clone + 2 * n_child
        if m >= 2 ** 31:
            raise ValueError(f"{what}: the new row count {m} reaches 2^31; the library indexes rows with 32 bits")
        if n_split:
            if noise is None:
                noise = torch.randn((2 * n_split, 3), generator=generator, dtype=torch.float32, device=dev)
            elif noise.shape[0] != 2 * n_split:
                raise ValueError(f"{what}: noise must be [2 * {n_split} split parents, 3], got {tuple(noise.shape)}")
        move = _lib.DensityMoveStruct()
        rows, new_data, new_moments = 0, {}, {}
        for name in GROUPS:
            src = data[name]
            width = int(torch.Size(src.shape[1:]).numel())
            srcs = [(src, _KIND.get(name, "copy"))]
            st = optimizer.state.get(by_name[name]["params"][0])
            if st:
                srcs += [(st["exp_avg"], "moment"), (st["exp_avg_sq"], "moment")]
            dsts = []
            for t, kind in srcs:
                dst = torch.empty((m,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
                dsts.append(dst)
                if width == 0:          # f_rest of SH degree 0: nothing to move
                    continue
                move.row[rows] = _lib.DensityRowStruct(t.data_ptr(), dst.data_ptr(), width, _lib.DENSITY_ROW[kind])
                rows += 1
            new_data[name], new_moments[name] = dsts[0], dsts[1:]
        kept_state = []
        if keep_state:
            for t in (state.xyz_gradient_accum, state.denom, state.max_radii2D):
                dst = torch.empty((m,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
                move.row[rows] = _lib.DensityRowStruct(t.data_ptr(), dst.data_ptr(), 1, _lib.DENSITY_ROW["copy"])
                rows += 1
                kept_state.append(dst)
        move.rows, move.n, move.action, move.rank = rows, n, action.data_ptr(), rank.data_ptr()
        move.n_kept, move.n_clone, move.n_split, move.n_child = n_kept, n_clone, n_split, n_child
        move.scaling, move.rotation = data["scaling"].data_ptr(), data["rotation"].data_ptr()
        move.noise = noise.data_ptr() if n_split else None
        _lib.call(lib.texgs_density_move, C.byref(move), stream)
    out = {}
    for name in GROUPS:         # the optimizer's state, edited as _prune_optimizer / cat_tensors_to_optimizer edit it (:200-254)
        group = by_name[name]
        old = group["params"][0]
        stored = optimizer.state.get(old, None)
        new = nn.Parameter(new_data[name].requires_grad_(True))
        if stored:
            stored["exp_avg"], stored["exp_avg_sq"] = new_moments[name]
            del optimizer.state[old]
            group["params"][0] = new
            optimizer.state[new] = stored
        else:
            group["params"][0] = new
        out[name] = new
    if keep_state:
        state.xyz_gradient_accum, state.denom, state.max_radii2D = kept_state
    else:
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        state.xyz_gradient_accum, state.denom, state.max_radii2D = z(m, 1), z(m, 1), z(m)
    return out


def densify_and_prune(params, optimizer, state, *, max_grad, min_opacity, extent, max_screen_size, percent_dense, noise=None,
                      generator=None):
    """models/gaussian3d.py:318-332 in one pass.  `params`: {"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"} -> the raw
    parameters held in `optimizer` (one per group, groups named so).  Returns the new parameters by name; `optimizer` holds them and
    their resized Adam moments (copied for surviving originals, zero for new rows), `state` is all zeros at the new size.

    With g = accum / denom (NaN -> 0), m = max exp(scaling), o = sigmoid(opacity): clone if g >= max_grad and m <= percent_dense
    extent; split into two children (scale / 1.6, position xyz + R (s * eps)) if g >= max_grad and m > percent_dense extent; the
    split parent goes.  An original, a clone or a pair of children is pruned if o < min_opacity or -- only when max_screen_size
    is truthy -- its m > 0.1 extent.  `max_screen_size` itself is never compared: the reference zeroes max_radii2D before it reads
    it (module docstring).  max_grad must be positive: with 0 the reference would split its own clones.
    `noise` f32[2 ns, 3]: the standard-normal samples of the split; None draws them with torch.randn(generator=generator)."""
    what = "densify_and_prune"
    max_grad, min_opacity = _number(max_grad, f"{what}: max_grad"), _number(min_opacity, f"{what}: min_opacity")
    extent, percent_dense = _number(extent, f"{what}: extent"), _number(percent_dense, f"{what}: percent_dense")
    if not max_grad > 0:
        raise ValueError(f"{what}: max_grad must be positive, got {max_grad} (with 0 the reference would split its own clones)")
    if max_screen_size is not None:
        _number(max_screen_size, f"{what}: max_screen_size")
    return _resize(what, params, optimizer, state, max_grad, min_opacity, percent_dense * extent, 0.1 * extent, True,
                   bool(max_screen_size), noise, generator)


def opacity_prune(params, optimizer, state, min_opacity):
    """models/gaussian3d.py:338-341: drop every Gaussian with sigmoid(opacity) < min_opacity.  The survivors' rows of the statistics
    are KEPT (prune_points masks them, :229-232), unlike after densify_and_prune: they are three more copied tensors of the move."""
    what = "opacity_prune"
    min_opacity = _number(min_opacity, f"{what}: min_opacity")
    return _resize(what, params, optimizer, state, 1.0, min_opacity, 0.0, 0.0, False, False, None, None, keep_state=True)


def reset_opacity(params, optimizer):
    """models/gaussian3d.py:180-183: opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), both moments of the group zeroed.
    Returns the new opacity parameter."""
    seen = []
    by_name, data, _ = _groups(params, optimizer, "reset_opacity", seen)
    _on_gpu(seen)
    o = torch.sigmoid(data["opacity"])
    x = torch.min(o, torch.ones_like(o) * 0.01)
    return _replace_tensor(optimizer, torch.log(x / (1 - x)), "opacity", "reset_opacity")


def reset_min_scale(params, optimizer):
    """models/gaussian3d.py:343-350: the smallest raw scale of every Gaussian (torch.argmin's choice on ties) becomes -20, both moments
    of the group zeroed.  Returns the new scaling parameter."""
    seen = []
    by_name, data, _ = _groups(params, optimizer, "reset_min_scale", seen)
    _on_gpu(seen)
    scaling_new = data["scaling"].clone()
    idx = torch.argmin(scaling_new, dim=1, keepdim=True)
    scaling_new.scatter_(1, idx, -20.0)
    return _replace_tensor(optimizer, scaling_new, "scaling", "reset_min_scale")


def _replace_tensor(optimizer, tensor, name, what):
    """replace_tensor_to_optimizer, models/gaussian3d.py:185-198: the new parameter with both moments zeroed"""
    for group in optimizer.param_groups:
        if group.get("name") == name:
            old = group["params"][0]
            stored = optimizer.state.get(old, None)
            new = nn.Parameter(tensor.requires_grad_(True))
            if stored:
                stored["exp_avg"] = torch.zeros_like(tensor)
                stored["exp_avg_sq"] = torch.zeros_like(tensor)
                del optimizer.state[old]
                group["params"][0] = new
                optimizer.state[new] = stored
            else:
                group["params"][0] = new
            return new
    raise KeyError(f"{what}: the optimizer has no group named {name!r}")
