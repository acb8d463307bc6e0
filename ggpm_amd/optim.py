"""Adam over one flat view of all parameters.

``vae_train.py:60`` uses ``torch.optim.Adam(model.parameters())``.  The update is elementwise, so running it on ONE
flat fp32 tensor that all parameters are views of gives the same numbers with one optimizer "parameter": one fused
launch and none of the per-parameter Python bookkeeping of a 39-tensor parameter list (~0.2 ms of host time per step,
which matters once the encoder step itself is ~2.5 ms and host bound).  Gradients come from
``ggpm_amd.parallel.FlatGradSync(keep_flat=True)``, whose flat buffer has the same layout: the C++ encoder backward
writes into it directly, so nothing is packed or copied for the optimizer either.

What the reference's training loops do around the optimizer runs on the same buffers:

* ``clip_grad_norm_(model.parameters(), clip_norm)`` (all four scripts) is ``step(clip_norm=...)``: one launch that leaves
  the sum of squares as per-workgroup partials and the Adam launch behind it, which forms the coefficient and uses
  ``g * coef``.  No host synchronisation: ``last_grad_norm`` / ``last_clip_coef`` are device tensors.
* the four optimizers of ``vae_fine_tune_indv_opt.py:61-70`` (one learning rate each, one ``ExponentialLR`` rate for all)
  are ``param_groups=[{"params": ..., "lr": ...}, ...]``: the kernel looks the hyper-parameters up per 64-float tile.
* the ``param_norm`` / ``grad_norm`` the scripts print are ``param_norm()`` / ``grad_norm()``: two launches each instead of
  one ``.item()`` per parameter.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _dev

MAX_GROUPS = 8              # GGPM_ADAM_MAX_GROUPS (include/ggpm_hip.h)


class AdamGroup(ctypes.Structure):      # ggpm_adam_group
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float)]


def _assign_groups(sync, param_groups):
    """``param_groups`` (torch's list of dicts) -> for every group the slots of ``sync.params`` it owns.  Every parameter of
    the sync belongs to exactly one group, by identity; a parameter listed twice in ONE group (a tied embedding reached through
    two modules) counts once."""
    if len(param_groups) < 1 or len(param_groups) > MAX_GROUPS:
        raise ValueError("FlatAdam: %d parameter groups; the step kernel takes 1 to %d" % (len(param_groups), MAX_GROUPS))
    slot_of = {id(p): i for i, p in enumerate(sync.params)}
    owner, slots = {}, []
    for k, grp in enumerate(param_groups):
        if not isinstance(grp, dict) or "params" not in grp:
            raise ValueError("FlatAdam: parameter group %d is not a dict with a 'params' entry" % k)
        ps = grp["params"]
        mine = []
        for p in ([ps] if isinstance(ps, torch.Tensor) else list(ps)):
            i = slot_of.get(id(p))
            if i is None:
                raise ValueError("FlatAdam: parameter group %d holds a parameter (shape %s) that is not in the FlatGradSync"
                                 % (k, tuple(p.shape)))
            if i in owner:
                if owner[i] != k:
                    raise ValueError("FlatAdam: parameter %d of the sync (shape %s) is in groups %d and %d"
                                     % (i, tuple(p.shape), owner[i], k))
                continue
            owner[i] = k
            mine.append(i)
        slots.append(sorted(mine))
    missing = [i for i in range(len(sync.params)) if i not in owner]
    if missing:
        raise ValueError("FlatAdam: %d parameter(s) of the sync are in no group (first: slot %d, shape %s)"
                         % (len(missing), missing[0], tuple(sync.params[missing[0]].shape)))
    return slots


class FlatAdam:
    """``FlatAdam(sync, lr, ...)``: torch.optim.Adam over the parameters of ``sync`` (a FlatGradSync with keep_flat=True).

    ``param_groups``: a list of dicts in torch's shape, ``{"params": iterable of Parameters, "lr": ...}`` with optional
    ``betas``, ``eps`` and ``weight_decay`` (missing keys take the constructor's values), at most 8.  ``opt`` is a
    torch.optim.Optimizer whose ``param_groups`` carry one entry per group: schedulers act on it and every step reads
    the current values from it.  One step count serves all groups.
    """

    def __init__(self, sync, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 param_groups=None):
        self.sync = sync
        params = sync.params
        param_groups = list(param_groups) if param_groups is not None else None
        slots = _assign_groups(sync, param_groups) if param_groups is not None else None
        # the gradient buffer's layout: every parameter on a 256-byte boundary (parallel.FlatGradSync says why), zeros between
        flat = torch.zeros(sync.flat.numel(), dtype=params[0].dtype, device=params[0].device)
        with torch.no_grad():
            for p, off in zip(params, sync.offsets):
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view_as(p)          # the module's parameters are views of the flat buffer now
        self.flat = torch.nn.Parameter(flat)
        self.grouped = slots is not None
        self._tile_group = None
        if not self.grouped:
            self.opt = torch.optim.Adam([self.flat], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=flat.is_cuda)
        else:
            groups = []
            for grp, mine in zip(param_groups, slots):
                groups.append(dict({k: v for k, v in grp.items() if k != "params"}, params=[params[i] for i in mine]))
            # the parameters themselves, for the torch-op form; the HIP step only reads the hyper-parameters of each group
            self.opt = torch.optim.Adam(groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=flat.is_cuda)
            # the group of every ALIGN-float tile of the flat buffers (a parameter's padding goes with the parameter)
            assert sync.ALIGN == 64 and flat.numel() % 64 == 0
            tiles = torch.zeros(flat.numel() // 64, dtype=torch.uint8)
            ends = list(sync.offsets[1:]) + [flat.numel()]
            for k, mine in enumerate(slots):
                for i in mine:
                    tiles[sync.offsets[i] // 64:ends[i] // 64] = k
            self._tile_group = tiles.to(flat.device)
        # on the GPU the step is ONE launch of ggpm_adam_step over the flat buffer (torch's fused Adam issues three
        # multi-tensor launches for it); learning-rate schedulers keep working through ``param_groups``
        self._hip = flat.is_cuda and _dev.HIP_ADAM
        self.last_grad_norm = self.last_clip_coef = None
        if self._hip:
            from . import _lib
            self._m, self._v, self._t = torch.zeros_like(flat), torch.zeros_like(flat), 0
            # workspace of the norm launches (caller-owned: a step allocates nothing) and where a clipped step leaves
            # {norm, coefficient}
            ws = int(_lib.load().ggpm_flat_sqnorm_workspace_bytes(flat.numel()))
            self._partials = torch.zeros(ws // 8, dtype=torch.float64, device=flat.device)
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=flat.device)
            self._clip_views = (self._clip_out[0], self._clip_out[1])
            self._groups_c = _lib.array_type(AdamGroup, MAX_GROUPS)()

    @property
    def param_groups(self):
        return self.opt.param_groups

    # ------------------------------------------------------------------ HIP form
    def _sqnorm_partials(self, lib, x: torch.Tensor) -> None:
        from . import _lib
        from . import functional as F_
        _lib.check(lib.ggpm_flat_sqnorm_partials(F_._p(x), x.numel(), F_._p(self._partials), self._partials.numel() * 8,
                                                 F_._stream()), "flat_sqnorm_partials")

    def _norm(self, x: torch.Tensor) -> torch.Tensor:
        if not self._hip:
            return torch.linalg.vector_norm(x.detach(), 2, dtype=torch.float64).to(x.dtype)
        from . import _lib
        from . import functional as F_
        lib = _lib.load()
        out = torch.empty(1, dtype=torch.float32, device=x.device)      # the caching allocator: no synchronisation
        self._sqnorm_partials(lib, x)
        _lib.check(lib.ggpm_flat_norm_finish(F_._p(self._partials), self._partials.numel(), 0.0, F_._p(out), F_._stream()),
                   "flat_norm_finish")
        return out[0]

    def grad_norm(self) -> torch.Tensor:
        """2-norm of the whole gradient (the scripts' ``math.sqrt(sum(p.grad.norm() ** 2))``) as a 0-dim device tensor: two
        launches, no synchronisation.  Call after ``sync.all_reduce()``; after ``step(clip_norm=...)`` without
        ``write_clipped`` this is still the norm before clipping."""
        return self._norm(self.sync.flat)

    def param_norm(self) -> torch.Tensor:
        """2-norm of all parameters (the scripts' ``math.sqrt(sum(p.norm() ** 2))``), as grad_norm()."""
        return self._norm(self.flat.data)

    def _step_hip(self, clip_norm, write_clipped: bool) -> None:
        from . import _lib
        from . import functional as F_
        lib = _lib.load()
        groups = self.opt.param_groups
        for c, grp in zip(self._groups_c, groups):
            c.lr, c.beta1, c.beta2 = float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1])
            c.eps, c.weight_decay = float(grp["eps"]), float(grp["weight_decay"])
        g = self.sync.flat
        clip = clip_norm is not None
        if clip:
            self._sqnorm_partials(lib, g)
        self._t += 1
        _lib.check(lib.ggpm_adam_step_groups(
            F_._p(self.flat.data), F_._p(g), F_._p(self._m), F_._p(self._v), self.flat.numel(), F_._p(self._tile_group),
            len(groups), ctypes.addressof(self._groups_c), self._t, F_._p(self._partials if clip else None),
            self._partials.numel() if clip else 0, float(clip_norm) if clip else 0.0, F_._p(self._clip_out if clip else None),
            int(bool(write_clipped)), F_._stream()), "adam_step_groups")
        if clip:
            self.last_grad_norm, self.last_clip_coef = self._clip_views

    # ------------------------------------------------------------------ step interface
    def step(self, clip_norm=None, write_clipped: bool = False) -> None:
        """Call after ``sync.all_reduce()`` (which also gathers stray gradients into the flat buffer on one rank).

        ``clip_norm``: the step is ``clip_grad_norm_(parameters, clip_norm)`` followed by the optimizer step, in two launches.
        ``last_grad_norm`` is then a 0-dim device tensor with the norm BEFORE clipping (what ``clip_grad_norm_`` returns) and
        ``last_clip_coef`` the coefficient ``min(clip_norm / (norm + 1e-6), 1)``; both are views of one buffer that the next
        clipped step overwrites, and neither synchronises until the caller reads it (``.item()``).

        On the HIP path the gradient buffer keeps the UNSCALED gradient unless ``write_clipped`` is set (then ``p.grad``
        reads as torch leaves it after ``clip_grad_norm_``, for one more store per element); the norm after clipping that the
        reference prints is ``last_grad_norm * last_clip_coef`` either way.  The torch-op form (a CPU buffer, or
        ``_dev.HIP_ADAM`` off) always scales the buffer in place, as torch does.
        """
        if clip_norm is not None and not float(clip_norm) > 0.0:
            raise ValueError("FlatAdam.step: clip_norm must be positive (got %r)" % (clip_norm,))
        if self._hip:
            if clip_norm is None and not self.grouped:
                from . import _lib
                from . import functional as F_
                g, grp = self.sync.flat, self.opt.param_groups[0]
                self._t += 1
                _lib.check(_lib.load().ggpm_adam_step(F_._p(self.flat.data), F_._p(g), F_._p(self._m), F_._p(self._v),
                                                      self.flat.numel(), float(grp["lr"]), float(grp["betas"][0]),
                                                      float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]),
                                                      self._t, F_._stream()), "adam_step")
                return
            self._step_hip(clip_norm, write_clipped)
            return
        # torch ops: torch.optim.Adam over the flat parameter, or per group over the parameters (views of the same buffers)
        if self.grouped:
            for p, v in zip(self.sync.params, self.sync.views):
                p.grad = v
            clipped = self.sync.params
        else:
            self.flat.grad = self.sync.flat
            clipped = [self.flat]
        if clip_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(clipped, float(clip_norm))
            self.last_grad_norm = norm
            self.last_clip_coef = torch.clamp(float(clip_norm) / (norm + 1e-6), max=1.0)
        self.opt.step()

    def zero_grad(self) -> None:
        self.sync.zero_grad()
