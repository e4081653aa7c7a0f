"""The optimizer phase of the reference's optimize_step (models/texture_gaussian3d.py:420-444, likewise gaussian3d.py and
uv_map_gaussian3d.py) in one pass (csrc/optim.hip, include/texgs_optim.h): three `torch.optim.Adam(..., eps=1e-15).step()` calls and the
`zero_grad` behind them.

* `FusedAdam` IS a `torch.optim.Adam`: the same constructor, the same param_groups, the same state (`step` a CPU float32 scalar,
  `exp_avg` / `exp_avg_sq` from zeros_like), so state_dict() / load_state_dict() interchange with a plain Adam in both directions and
  texgs.density edits it as it edits torch's.  Only step() differs: every participating tensor is one 64-byte record of ONE
  texgs_adam_step call per device, which moves 28 bytes per element (32 with zero_grads) where the foreach path makes several
  element-wise passes with temporaries.
* `fused_step([optimizer, optimizer_uv, optimizer_tex], zero_grads=True)` steps several FusedAdam instances through one call.

The arithmetic is a contract (tests/adam_ref.py states it in numpy, the GPU tests compare bit for bit): per element, one fp32 rounding
per operation, in torch's single-tensor order
    d  = g - m;          m' = (w1 < 0.5) ? m + w1*d : g - d*(1 - w1)       # exp_avg.lerp_(grad, 1 - beta1)
    v' = v*beta2;        v' = v' + (w2*g)*g                                # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    den = sqrt(v')/bc2_sqrt + eps
    p' = p + neg_step_size*(m'/den)                                        # param.addcdiv_(exp_avg, denom, value=-step_size)
with the scalars prepared in Python doubles from each tensor's own `step` and rounded to fp32 once (`scalars`).

Not supported, refused by name: weight_decay, amsgrad, maximize, capturable, differentiable, fused.  No CPU fallback: CPU tensors raise.
Nothing is read back from the device and nothing is allocated after the first step of a parameter."""
import ctypes as C

import torch

from . import _lib

CHUNK = 1024            # TEXGS_ADAM_CHUNK: elements one workgroup updates at a time
MAX_TENSORS = 32        # TEXGS_ADAM_MAX_TENSORS: records per launch
_f32 = lambda x: C.c_float(x).value


class AdamTensor(C.Structure):
    """ctypes mirror of TexGSAdamTensor (include/texgs_optim.h), 64 bytes"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_int64),
                ("w1", C.c_float), ("beta2", C.c_float), ("w2", C.c_float), ("bc2_sqrt", C.c_float), ("eps", C.c_float),
                ("neg_step_size", C.c_float)]


# the entry point's signature: (restype, argtypes) of `int texgs_adam_step(const TexGSAdamTensor*, int32_t, int32_t, void*)`
SIGNATURE = (C.c_int, [C.POINTER(AdamTensor), C.c_int32, C.c_int32, C.c_void_p])
_SIGNATURES = {"texgs_adam_step": SIGNATURE}


def entry():
    """texgs_adam_step of the loaded library with its signature applied (on first use)"""
    return _lib.bind(_SIGNATURES).texgs_adam_step


def scalars(step, lr, betas, eps):
    """The six fp32 scalars of a record, from Python doubles as torch's single-tensor Adam computes them, each rounded to fp32 once:
    (w1, beta2, w2, bc2_sqrt, eps, neg_step_size)"""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step, lr = float(step), float(lr)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    return (_f32(1 - beta1), _f32(beta2), _f32(1 - beta2), _f32(bias_correction2 ** 0.5), _f32(float(eps)), _f32(-step_size))


_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


def _check_group(group):
    """(the first line is the whole cost of a group that is fine: this runs for every group of every step)"""
    get = group.get
    if not (get("weight_decay", 0) != 0 or get("amsgrad") or get("maximize") or get("capturable") or get("differentiable")
            or get("fused") or isinstance(group["lr"], torch.Tensor) or isinstance(group["eps"], torch.Tensor)
            or isinstance(group["betas"][0], torch.Tensor) or isinstance(group["betas"][1], torch.Tensor)):
        return
    if get("weight_decay", 0) != 0:
        raise ValueError(f"FusedAdam does not support weight_decay (got {group['weight_decay']}); use torch.optim.Adam for it")
    for k in _REFUSED:
        if get(k):
            raise ValueError(f"FusedAdam does not support {k}={group[k]!r}; use torch.optim.Adam for it")
    for k, x in (("lr", group["lr"]), ("eps", group["eps"]), ("betas[0]", group["betas"][0]), ("betas[1]", group["betas"][1])):
        if isinstance(x, torch.Tensor) and x.device.type != "cpu":
            raise ValueError(f"FusedAdam: {k} is a tensor on {x.device}; reading it would synchronise -- pass a number or a CPU tensor")


def _fault(t):
    """Why a tensor cannot take part in a step, as (exception class, text), or None"""
    if t.layout is not torch.strided:
        return RuntimeError, "is sparse; only dense tensors are supported"
    if t.dtype is not torch.float32:
        return ValueError, f"must be torch.float32, got {t.dtype}"
    if not t.is_contiguous():
        return ValueError, "must be contiguous"
    return None


_ROLE = ("", "the gradient of ", "exp_avg of ", "exp_avg_sq of ")


def _name(role, pi, gi, group):
    """(built only when something is refused)"""
    return f"{_ROLE[role]}parameter {pi} of group {group.get('name', gi)!r}"


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() is one texgs_adam_step call (module docstring).  `foreach` is accepted and ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _check_group(dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                          capturable=capturable, differentiable=differentiable, fused=fused))
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=foreach,
                         maximize=maximize, capturable=capturable, differentiable=differentiable, fused=fused,
                         decoupled_weight_decay=decoupled_weight_decay)
        for group in self.param_groups:
            _check_group(group)

    def _gather(self):
        """Every check of a step: -> [(p, group)] of the parameters that have a gradient.  Nothing is launched, made or advanced here.
        Per parameter: layout and dtype of the parameter, its gradient and its moments, then their shapes, then their devices."""
        work = []
        states = self.state
        for gi, group in enumerate(self.param_groups):
            _check_group(group)
            for pi, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                state = states.get(p)                   # (a defaultdict: asking it with [] would make the entry)
                if state:
                    for k in ("exp_avg", "exp_avg_sq"):
                        if not isinstance(state.get(k), torch.Tensor):
                            raise ValueError(f"FusedAdam: the state of {_name(0, pi, gi, group)} has no {k}")
                    tensors = (p, g, state["exp_avg"], state["exp_avg_sq"])
                else:
                    tensors = (p, g)
                for role, t in enumerate(tensors):
                    bad = _fault(t)
                    if bad:
                        raise bad[0](f"FusedAdam: {_name(role, pi, gi, group)} {bad[1]}")
                shape = p.shape
                for role, t in enumerate(tensors):
                    if t.shape != shape:
                        raise ValueError(f"FusedAdam: {_name(role, pi, gi, group)} has shape {tuple(t.shape)}, the parameter {tuple(shape)}")
                if state:
                    step = state.get("step")
                    if step is None:
                        raise ValueError(f"FusedAdam: the state of {_name(0, pi, gi, group)} has no step")
                    if isinstance(step, torch.Tensor) and step.is_cuda:
                        raise ValueError(f"FusedAdam: step of {_name(0, pi, gi, group)} is on {step.device}; reading it would "
                                         "synchronise (a capturable or fused torch.optim.Adam state?)")
                index = p.get_device()                  # -1 for a CPU tensor
                for role, t in enumerate(tensors):
                    if not t.is_cuda:
                        raise RuntimeError(f"FusedAdam: {_name(role, pi, gi, group)} must be on an AMD GPU; there is no CPU fallback")
                    if t.get_device() != index:         # (parameters on several GPUs are fine: one call per device)
                        raise ValueError(f"FusedAdam: {_name(0, pi, gi, group)}, its gradient and its moments span devices: "
                                         f"{sorted({str(x.device) for x in tensors})}")
                work.append((p, group))
        return work

    def _state_of(self, p):
        """The parameter's state, made on its first step as torch's single-tensor path makes it (Adam._init_group)"""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @torch.no_grad()
    def step(self, closure=None, zero_grads=False):
        """One Adam step of every parameter that has a gradient.  zero_grads=True also stores +0.0 to those gradients in the same
        pass (what zero_grad(set_to_none=False) would do afterwards).  One launch per 32 tensors and device, on the current stream."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _launch(_records([self]), zero_grads)
        return loss


def _records(optimizers):
    """Checks everything of every optimizer first, then advances the step counters and builds the records: {device index: [AdamTensor]}"""
    for o in optimizers:
        if not isinstance(o, FusedAdam):
            raise TypeError(f"fused_step: expected texgs.optim.FusedAdam instances, got {type(o).__name__}")
    works = [o._gather() for o in optimizers]
    by_device, known = {}, {}
    for o, work in zip(optimizers, works):
        for p, group in work:
            state = o._state_of(p)
            step = state["step"]
            step += 1                   # in place, like torch: the tensor in the state is the counter
            key = (float(step), group["lr"], group["betas"][0], group["betas"][1], group["eps"])
            sc = known.get(key)
            if sc is None:              # the tensors of a group, and often of an optimizer, share their scalars
                sc = known[key] = scalars(key[0], key[1], key[2:4], key[4])
            recs = by_device.get(p.get_device())
            if recs is None:
                recs = by_device[p.get_device()] = []
            recs.append(AdamTensor(p.data_ptr(), p.grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(),
                                   p.numel(), *sc))
    return by_device


def _launch(by_device, zero_grads):
    fn = entry() if by_device else None
    for index, recs in by_device.items():
        arr = (AdamTensor * len(recs))(*recs)
        with _lib.on(torch.device("cuda", index)) as stream:
            _lib.call(fn, arr, len(recs), 1 if zero_grads else 0, stream)


@torch.no_grad()
def fused_step(optimizers, zero_grads=False):
    """Steps several FusedAdam instances -- the reference's `optimizer`, `optimizer_uv`, `optimizer_tex` -- through ONE texgs_adam_step
    call per device and advances each one's step counters.  Learning rates are read from param_groups now, so schedulers and
    update_learning_rate work unchanged.  Every check of every optimizer is made before anything changes."""
    optimizers = list(optimizers)
    _launch(_records(optimizers), zero_grads)
    for o in optimizers:
        o._opt_called = True            # what a torch lr_scheduler's wrapper of step() records
