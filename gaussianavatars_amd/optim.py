"""Fused Adam step (include/gop.h): `optimizer.step()` of the reference's loop (train.py:209) as ONE launch for every parameter group.

    FusedAdam(params, lr=..., eps=...)     a torch.optim.Adam whose step() is gop_adam_step_ex
    adopt(optimizer)                       turns a live, plain torch.optim.Adam into one, in place (patch.patch_optimizer)

The class overrides step() and nothing else.  Its state is torch's own -- per parameter {"step": CPU scalar tensor, "exp_avg",
"exp_avg_sq"}, created by torch.optim.Adam._init_group itself, so exactly where and how torch creates it -- which is why
state_dict() / load_state_dict() interchange with torch.optim.Adam and why the reference's surgery on `optimizer.state`
(replace_tensor_to_optimizer, _prune_optimizer, cat_tensors_to_optimizer: scene/gaussian_model.py:334-424), capture() / restore() and
gaussian_model.spatial_resort work untouched.  `step` stays a host scalar, so the two bias corrections of every tensor are formed on the
host, in double, as torch forms them, and ride in the kernel arguments: the step reads nothing back from the device.

Semantics kept: a parameter whose .grad is None is skipped and its step does not advance (every splat parameter on a densification
iteration: train.py:202 replaces them before :209 steps); every group's lr is read at step time; betas / eps are per group (groups whose
(beta1, beta2, eps) differ go in separate launches); every tensor carries its own step count.

The WHOLE step is torch's own Adam.step, bit for bit, whenever anything is outside the kernel's domain: a closure; amsgrad, weight_decay,
maximize, capturable, differentiable, fused or decoupled_weight_decay on any group; a tensor lr; a parameter, gradient or moment that is
not a contiguous fp32 tensor of one GPU (CPU tensors, other dtypes, non-contiguous or sparse gradients); a stream that is being captured
(the bias corrections would be frozen into the recorded kernel arguments).  That is a statement about the domain, not a quiet substitute
for a missing kernel: inside the domain a missing libgop_hip.so is an error.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["FusedAdam", "adopt"]

_UNSUPPORTED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay")


def _torch_step(opt, closure):
    """torch.optim.Adam.step without the profiling / hook wrapper Optimizer.__init__ puts around it (FusedAdam.step runs inside its own)."""
    fn = torch.optim.Adam.step
    if getattr(fn, "hooked", False) and hasattr(fn, "__wrapped__"):
        fn = fn.__wrapped__
    return fn(opt, closure)


def _dense_f32(t, dev) -> bool:
    return t.dtype is torch.float32 and t.device == dev and t.layout is torch.strided and t.is_contiguous()


class FusedAdam(torch.optim.Adam):
    __doc__ = __doc__

    def _in_domain(self):
        """The device every participating tensor lives on; None when the step has to be torch's own; False when nothing has a gradient."""
        dev = None
        for group in self.param_groups:
            if group["weight_decay"] != 0 or any(group.get(f) for f in _UNSUPPORTED_FLAGS):
                return None
            if not isinstance(group["lr"], (int, float)) or not all(isinstance(b, float) for b in group["betas"]):
                return None
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if dev is None:
                    dev = p.device
                    if dev.type != "cuda":
                        return None
                if not _dense_f32(p, dev) or not _dense_f32(g, dev) or g.numel() != p.numel():
                    return None
        if dev is None:
            return False
        return None if torch.cuda.is_current_stream_capturing() else dev

    @torch.no_grad()
    def step(self, closure=None):
        dev = None if closure is not None else self._in_domain()
        if dev is None:
            return _torch_step(self, closure)
        if dev is False:      # no gradient anywhere: torch's step creates no state and advances nothing
            return None
        work = []             # (group, params, grads, exp_avgs, exp_avg_sqs, steps)
        for group in self.param_groups:
            lists = ([], [], [], [], [], [])
            self._init_group(group, *lists)   # torch's own lazy state creation
            params, grads, exp_avgs, exp_avg_sqs, _, steps = lists
            for p, m, v, s in zip(params, exp_avgs, exp_avg_sqs, steps):
                if not (_dense_f32(m, dev) and _dense_f32(v, dev) and m.numel() == p.numel() == v.numel() and s.device.type == "cpu"):
                    return _torch_step(self, None)   # (state loaded from elsewhere; nothing has been advanced yet)
            if params:
                work.append((group, params, grads, exp_avgs, exp_avg_sqs, steps))
        launches = {}         # (beta1, beta2, eps) -> rows of the descriptor table
        for group, params, grads, exp_avgs, exp_avg_sqs, steps in work:
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            rows = launches.setdefault((beta1, beta2, group["eps"]), [])
            for p, g, m, v, s in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
                s += 1
                t = s.item()
                rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                             lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5))
        lib = _lib.gop()
        with _lib.on_device(dev):
            stream = _lib.raw_stream(dev)
            for (beta1, beta2, eps), rows in launches.items():
                table = (_lib.GopAdamTensor * len(rows))(*rows)
                if lib.gop_adam_step_ex(len(rows), table, beta1, 1 - beta1, beta2, 1 - beta2, eps, stream) != 0:
                    raise RuntimeError(f"gop_adam_step_ex failed: {_lib.gop_error()}")
        return None


def adopt(optimizer):
    """Turns a plain torch.optim.Adam into a FusedAdam in place -- the same object, the same param_groups, the same state -- and returns it.
    Anything that is not exactly torch.optim.Adam (a subclass, another optimizer, a FusedAdam) is returned unchanged."""
    if type(optimizer) is not torch.optim.Adam:
        return optimizer
    optimizer.__class__ = FusedAdam
    optimizer._patch_step_function()   # the profiling / hook wrapper around the new class's step(), as Optimizer.__init__ installs it
    return optimizer
