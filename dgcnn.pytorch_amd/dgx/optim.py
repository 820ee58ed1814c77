"""torch.optim.SGD / Adam / AdamW with their update in one HIP launch, and a
GradScaler whose inf check is one (libdgx.so dgx_sgd_step_f32,
dgx_sgd_step_amp_f32, dgx_adam_step_f32, dgx_amp_unscale_f32).

Same constructors, hyper-parameters, state (``state[p]["momentum_buffer"]``;
``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``) and update as
``torch.optim.SGD`` (torch/optim/sgd.py) and ``torch.optim.Adam`` / ``AdamW``
(torch/optim/adam.py, the single-tensor form), for fp32 parameters on a
ROCm device. torch's fused / foreach forms split a parameter list into
65536-element chunks with one workgroup each — a DGCNN's ~0.6 M parameters
run on ~22 workgroups, ~28 us per step at cfg2; here the whole list is one
grid-stride launch (48 tensors per launch). The training scripts of the
reference construct torch.optim.SGD / Adam (main_cls.py, main_semseg.py) or
AdamW (main_partseg_dist.py); these classes are drop-ins for them. State dicts
pass between a class here and torch's optimizer of the same kind in both
directions. Adam's ``step`` is kept as torch's fused form keeps it, a 0-dim
fp32 tensor on the parameter's device (a ``step`` loaded from a host-side
torch state is moved there at the next ``step()``), and is advanced on the
device by a one-workgroup launch after the update.

Capture. ``step()`` is capturable in a HIP graph once the state exists (after
the first eager step), with FIXED hyper-parameters: lr, momentum, dampening,
betas, eps and weight decay are kernel arguments, so a scheduler's change to
them reaches eager steps but not an already captured graph (recapture after
changing them). The exception is Adam / AdamW's ``lr`` given as a 0-dim fp32
device tensor: the kernel reads it, so ``lr.fill_(...)`` between replays takes
effect. (A float ``lr`` is rounded to fp32 on the way to the kernel, so both
forms give the same bits.) Parameters of one group may live on several
devices: each launch takes one device's tensors.

GradScaler. The three classes set ``_step_supports_amp_scaling``:
``GradScaler.step`` leaves ``grad_scale`` / ``found_inf`` on the optimizer and
the kernels take them as device pointers — the gradient is divided by the
scale on load (``.grad`` stays scaled, as with torch's fused optimizers) and a
non-zero ``found_inf`` makes the launch write nothing, step counts included.
No ``found_inf.item()``: the step costs no host synchronisation. SGD's
momentum buffers are created on the first step even if that step is skipped,
and the next step then takes the running-average form, as in torch's
``_fused_sgd``; torch leaves such a buffer uninitialised, here it is zero (so
the next step's buffer is ``(1 - dampening) * g``). ``dgx.optim.GradScaler``
is ``torch.amp.GradScaler`` with the unscale-and-check of fp32 device
gradients in one launch per 48 tensors."""
import ctypes
import types

import torch
from torch.amp.grad_scaler import _MultiDeviceReplicator

from . import _native as nat

_MAX = 48
_F32 = torch.float32


def _refuse(p, who):
    """The kernels take dense contiguous fp32 device tensors; anything else is an error, never another path."""
    if p.dtype != _F32 or p.grad.dtype != _F32 or not p.is_cuda:
        raise TypeError(f"dgx.optim.{who}: fp32 parameters on a ROCm device expected")
    if p.grad.is_sparse:
        raise RuntimeError(f"dgx.optim.{who}: sparse gradients are not supported")
    if not (p.is_contiguous() and p.grad.is_contiguous()):
        raise RuntimeError(f"dgx.optim.{who}: contiguous parameters and gradients expected")


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _numels(tensors):
    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


class _AmpState:
    """``optimizer.grad_scale`` / ``optimizer.found_inf`` as GradScaler.step sets them, per device."""

    def __init__(self, opt):
        self.grad_scale = getattr(opt, "grad_scale", None)
        self.found_inf = getattr(opt, "found_inf", None)
        self.active = self.grad_scale is not None or self.found_inf is not None
        self._on = {}

    def on(self, dev):
        """(grad_scale, found_inf) tensors on ``dev`` (kept alive by the caller until after the launch)."""
        if dev not in self._on:
            self._on[dev] = tuple(None if t is None else t.to(device=dev, dtype=_F32, non_blocking=True)
                                  for t in (self.grad_scale, self.found_inf))
        return self._on[dev]


class SGD(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *,
                 maximize=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = nat.lib()
        amp = _AmpState(self)
        for group in self.param_groups:
            mom = float(group["momentum"])
            # (first step of a buffer, parameter) lists: torch sets buf = d_p on a
            # parameter's first step, momentum * buf + (1 - dampening) * d_p after
            jobs = {}   # (first step, device) -> [(param, buffer)]: one launch per device
            for p in group["params"]:
                if p.grad is None:
                    continue
                _refuse(p, "SGD")
                first = False
                buf = None
                if mom != 0.0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        # under a scaler this step may write nothing: the buffer must not stay uninitialised
                        buf = (torch.zeros_like if amp.active else torch.empty_like)(
                            p, memory_format=torch.contiguous_format)
                        st["momentum_buffer"] = buf
                        first = True
                jobs.setdefault((first, p.device), []).append((p, buf))
            for (first, dev), lst in jobs.items():
                for c in range(0, len(lst), _MAX):
                    chunk = lst[c:c + _MAX]
                    n = len(chunk)
                    ps = _ptrs([p for p, _ in chunk])
                    gs = _ptrs([p.grad for p, _ in chunk])
                    ms = (ctypes.c_void_p * n)(*[(b.data_ptr() if b is not None else 0) for _, b in chunk])
                    ns = _numels([p for p, _ in chunk])
                    hyper = (float(group["lr"]), float(group["weight_decay"]), mom, float(group["dampening"]),
                             int(group["nesterov"]), int(group["maximize"]), int(first))
                    with torch.cuda.device(dev):
                        if amp.active:
                            scale, inf = amp.on(dev)
                            nat.check(lib.dgx_sgd_step_amp_f32(n, ps, gs, ms if mom != 0.0 else None, ns, *hyper,
                                                               nat.f32(scale), nat.f32(inf),
                                                               nat.stream_of(chunk[0][0])), "sgd step")
                        else:
                            nat.check(lib.dgx_sgd_step_f32(n, ps, gs, ms if mom != 0.0 else None, ns, *hyper,
                                                           nat.stream_of(chunk[0][0])), "sgd step")
        return loss


class Adam(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # there is one implementation here: torch's switches between its own are accepted only when unset
        for name, val in (("foreach", foreach), ("fused", fused), ("capturable", capturable),
                          ("differentiable", differentiable)):
            if val:
                raise ValueError(f"dgx.optim.{type(self).__name__}: {name}={val!r} is not supported "
                                 "(the update is always one HIP launch, capturable once the state exists)")
        # torch's keys, so that a state dict loads into torch.optim.Adam / AdamW and back
        super().__init__(params, dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps,
                                      weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                                      capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _state_of(self, p, amsgrad):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=_F32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if amsgrad:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            return st
        step = st["step"]
        if not (isinstance(step, torch.Tensor) and step.device == p.device and step.dtype == _F32):
            # torch's single-tensor / foreach forms keep it on the host
            st["step"] = torch.as_tensor(step).to(device=p.device, dtype=_F32).reshape(())
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = nat.lib()
        amp = _AmpState(self)
        who = type(self).__name__
        for group in self.param_groups:
            amsgrad = bool(group["amsgrad"])
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            jobs = {}   # device -> [(param, state)]: one launch per device
            for p in group["params"]:
                if p.grad is None:
                    continue
                _refuse(p, who)
                jobs.setdefault(p.device, []).append((p, self._state_of(p, amsgrad)))
            for dev, lst in jobs.items():
                lr_dev = None
                if isinstance(lr, torch.Tensor):
                    lr_dev = lr.to(device=dev, dtype=_F32, non_blocking=True)
                scale, inf = amp.on(dev)
                for c in range(0, len(lst), _MAX):
                    chunk = lst[c:c + _MAX]
                    with torch.cuda.device(dev):
                        nat.check(lib.dgx_adam_step_f32(
                            len(chunk), _ptrs([p for p, _ in chunk]), _ptrs([p.grad for p, _ in chunk]),
                            _ptrs([s["exp_avg"] for _, s in chunk]), _ptrs([s["exp_avg_sq"] for _, s in chunk]),
                            _ptrs([s["max_exp_avg_sq"] for _, s in chunk]) if amsgrad else None,
                            _ptrs([s["step"] for _, s in chunk]), _numels([p for p, _ in chunk]),
                            0.0 if lr_dev is not None else float(lr), nat.f32(lr_dev), float(beta1), float(beta2),
                            float(group["eps"]), float(group["weight_decay"]),
                            int(bool(group["decoupled_weight_decay"])), int(amsgrad), int(bool(group["maximize"])),
                            nat.f32(scale), nat.f32(inf), nat.stream_of(chunk[0][0])), "adam step")
        return loss


class AdamW(Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused,
                         decoupled_weight_decay=True)

    def __setstate__(self, state):   # as torch.optim.AdamW: whatever is loaded, the decay stays decoupled
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler with ``_unscale_grads_`` (the unscale and inf check of
    ``unscale_`` and ``step``) in one launch per 48 fp32 device gradients; any
    other gradient (fp16, sparse, host, non-contiguous) takes torch's path."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        per_device_inv_scale = _MultiDeviceReplicator(inv_scale)
        per_device_found_inf = _MultiDeviceReplicator(found_inf)
        ours, rest = {}, []
        for group in optimizer.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if (not allow_fp16) and g.dtype == torch.float16:
                    raise ValueError("Attempting to unscale FP16 gradients.")
                if g.dtype == _F32 and g.is_cuda and g.layout == torch.strided and g.is_contiguous():
                    ours.setdefault(g.device, []).append(g)
                else:
                    rest.append(p)
        lib = nat.lib() if ours else None
        with torch.no_grad():
            for dev, grads in ours.items():
                inv, inf = per_device_inv_scale.get(dev), per_device_found_inf.get(dev)
                with torch.cuda.device(dev):
                    for c in range(0, len(grads), _MAX):
                        chunk = grads[c:c + _MAX]
                        nat.check(lib.dgx_amp_unscale_f32(len(chunk), _ptrs(chunk), _numels(chunk), nat.f32(inv),
                                                          nat.f32(inf), nat.stream_of(chunk[0])), "amp unscale")
            found = per_device_found_inf._per_device_tensors
            if rest:   # the parent makes per-device flags of its own: fold them into ours
                theirs = super()._unscale_grads_(types.SimpleNamespace(param_groups=[{"params": rest}]), inv_scale,
                                                 found_inf, allow_fp16)
                for dev, flag in theirs.items():
                    if dev in found:
                        torch.maximum(found[dev], flag, out=found[dev])
                    else:
                        found[dev] = flag
        return found
