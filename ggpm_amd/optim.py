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
* checkpoints (``vae_train.py``'s ``save_iter`` / ``load_epoch``) are ``state_dict()`` / ``load_state_dict()`` in
  ``torch.optim.Adam``'s per-parameter format; ``skip_nonfinite`` refuses a step whose gradient norm is not finite, decided on
  the device in the same two launches; ``ema_decay`` keeps an exponential moving average of the parameters as one more stream
  of the update launch, and ``ema_weights()`` swaps it in for evaluation.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import struct

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


def _f32(x: float) -> float:
    """``x`` rounded to fp32 (round to nearest even), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


# keys of a torch param_group that choose an implementation, not a hyper-parameter: a loaded dict does not change them
_IMPL_KEYS = ("params", "fused", "foreach", "capturable", "differentiable")


class FlatAdam:
    """``FlatAdam(sync, lr, ...)``: torch.optim.Adam over the parameters of ``sync`` (a FlatGradSync with keep_flat=True).

    ``param_groups``: a list of dicts in torch's shape, ``{"params": iterable of Parameters, "lr": ...}`` with optional
    ``betas``, ``eps`` and ``weight_decay`` (missing keys take the constructor's values), at most 8.  ``opt`` is a
    torch.optim.Optimizer whose ``param_groups`` carry one entry per group: schedulers act on it and every step reads
    the current values from it.  One step count serves all groups.

    ``skip_nonfinite``: a step whose fp32 gradient norm (``last_grad_norm``) is not finite -- an Inf or a NaN anywhere in the
    gradient, or a finite gradient whose 2-norm overflows fp32 -- changes nothing: not the parameters, not the moments, not the
    EMA, not the gradient buffer, and Adam's step count does not advance (torch's Adam with ``optimizer.step()`` not called).
    The decision is taken on the device; ``last_step_skipped`` is a 0-dim device tensor (0 / 1), ``skipped_steps`` and
    ``applied_steps`` read the counter and may synchronise.

    ``ema_decay``: an exponential moving average of the parameters in ``ema`` (flat, the parameters' layout; ``ema_views`` per
    parameter), updated behind every applied step: ``e += (1 - d)(p - e)``, ``d = ema_decay`` or with ``ema_warmup``
    ``min(ema_decay, (1 + t) / (10 + t))``, t the count of applied steps.  ``with opt.ema_weights():`` runs its body with the
    averaged weights in the model.  With either feature the HIP step is still at most two launches (ggpm_adam_step_ex behind
    the partials); with neither it is the launches it was.

    ``state_dict()`` / ``load_state_dict()`` speak torch.optim.Adam's per-parameter format (see there).
    """

    def __init__(self, sync, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 param_groups=None, skip_nonfinite: bool = False, ema_decay=None, ema_warmup: bool = False):
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("FlatAdam: ema_decay must be in [0, 1) (got %r)" % (ema_decay,))
        if ema_warmup and ema_decay is None:
            raise ValueError("FlatAdam: ema_warmup without ema_decay")
        self.sync = sync
        params = sync.params
        param_groups = list(param_groups) if param_groups is not None else None
        slots = _assign_groups(sync, param_groups) if param_groups is not None else None
        # the slots of sync.params every group owns; torch numbers the parameters of a state dict in this order
        self._slots = slots if slots is not None else [list(range(len(params)))]
        self._order = [i for mine in self._slots for i in mine]
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
        self.last_grad_norm = self.last_clip_coef = self.last_step_skipped = None
        self.skip_nonfinite, self.ema_warmup = bool(skip_nonfinite), bool(ema_warmup)
        self.ema_decay = None if ema_decay is None else _f32(float(ema_decay))      # the kernel takes it as a float
        self._ex = self.skip_nonfinite or self.ema_decay is not None
        self._skipped = 0                                   # the torch-op form's count of skipped steps (HIP: on the device)
        self.ema = self.ema_views = None
        if self.ema_decay is not None:
            self.ema = torch.zeros_like(flat)
            self.ema_views = [self.ema[off:off + p.numel()].view_as(p) for p, off in zip(params, sync.offsets)]
            self.reset_ema()
        if self._hip and self._ex:
            # {norm, coef, skipped, t_eff} of the last step, and the skipped-step counter: two ints used in turn, the
            # step reads [_skip_cur] and writes the other
            self._status = torch.zeros(4, dtype=torch.float32, device=flat.device)
            self._status_views = (self._status[0], self._status[1], self._status[2])
            self._skip_ctr = torch.zeros(2, dtype=torch.int32, device=flat.device)
            self._ctr_views, self._skip_cur = (self._skip_ctr[0:1], self._skip_ctr[1:2]), 0
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

    def _fill_groups(self):
        """The current hyper-parameters of ``opt.param_groups`` into the ggpm_adam_group array the grouped launches read."""
        groups = self.opt.param_groups
        for c, grp in zip(self._groups_c, groups):
            c.lr, c.beta1, c.beta2 = float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1])
            c.eps, c.weight_decay = float(grp["eps"]), float(grp["weight_decay"])
        return groups

    def _step_hip(self, clip_norm, write_clipped: bool) -> None:
        from . import _lib
        from . import functional as F_
        lib = _lib.load()
        groups = self._fill_groups()
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

    def _step_ex(self, clip_norm, write_clipped: bool) -> None:
        """The step with the guard and / or the EMA: the partials (when the norm is needed) and ggpm_adam_step_ex."""
        from . import _lib
        from . import functional as F_
        lib = _lib.load()
        groups = self._fill_groups()
        g = self.sync.flat
        clip = clip_norm is not None
        need_norm = clip or self.skip_nonfinite
        if need_norm:
            self._sqnorm_partials(lib, g)
        self._t += 1
        cur = self._skip_cur
        _lib.check(lib.ggpm_adam_step_ex(
            F_._p(self.flat.data), F_._p(g), F_._p(self._m), F_._p(self._v), self.flat.numel(), F_._p(self._tile_group),
            len(groups), ctypes.addressof(self._groups_c), self._t, F_._p(self._partials if need_norm else None),
            self._partials.numel() if need_norm else 0, float(clip_norm) if clip else 0.0, int(bool(write_clipped)),
            F_._p(self.ema), self.ema_decay if self.ema is not None else 0.0, int(self.ema_warmup), int(self.skip_nonfinite),
            F_._p(self._ctr_views[cur]), F_._p(self._ctr_views[1 - cur]), F_._p(self._status), F_._stream()), "adam_step_ex")
        self._skip_cur = 1 - cur
        if need_norm:
            self.last_grad_norm = self._status_views[0]
        if clip:
            self.last_clip_coef = self._status_views[1]
        self.last_step_skipped = self._status_views[2]

    def _step_torch_ex(self, clip_norm) -> None:
        """The guard and the EMA with torch ops (the gradients are attached already).  The norm is formed as the kernels form it:
        accumulated in fp64, rounded to fp32 -- so the same gradients are refused in both forms.  Synchronises."""
        g = self.sync.flat
        clip = clip_norm is not None
        if clip or self.skip_nonfinite:
            norm = self._norm(g)
            self.last_grad_norm = norm
            if clip:
                coef = torch.clamp(float(clip_norm) / (norm + 1e-6), max=1.0)
                self.last_clip_coef = coef
            skipped = self.skip_nonfinite and not bool(torch.isfinite(norm))
            self.last_step_skipped = torch.full((), 1.0 if skipped else 0.0, dtype=torch.float32, device=g.device)
            if skipped:
                self._skipped += 1
                return
            if clip:
                g.mul_(coef)
        else:
            self.last_step_skipped = torch.zeros((), dtype=torch.float32, device=g.device)
        self.opt.step()
        if self.ema is not None:
            d = self.ema_decay
            if self.ema_warmup:
                t = self._applied_torch()
                d = min(d, _f32((1.0 + t) / (10.0 + t)))
            with torch.no_grad():
                self.ema.add_(self.flat.data - self.ema, alpha=_f32(1.0 - d))

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

        With ``skip_nonfinite`` the norm is formed on every step (``last_grad_norm`` is set without a clip too) and
        ``last_step_skipped`` is a 0-dim device tensor, 1 where this call changed nothing.
        """
        if clip_norm is not None and not float(clip_norm) > 0.0:
            raise ValueError("FlatAdam.step: clip_norm must be positive (got %r)" % (clip_norm,))
        if self._hip and self._ex:
            self._step_ex(clip_norm, write_clipped)
            return
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
        if self._ex:
            self._step_torch_ex(clip_norm)
            return
        if clip_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(clipped, float(clip_norm))
            self.last_grad_norm = norm
            self.last_clip_coef = torch.clamp(float(clip_norm) / (norm + 1e-6), max=1.0)
        self.opt.step()

    def zero_grad(self) -> None:
        self.sync.zero_grad()

    # ------------------------------------------------------------------ counters
    def _applied_torch(self) -> int:
        """Adam's step count of the torch-op form: the ``step`` torch keeps (one parameter's: all of them step together)."""
        st = self.opt.state.get(self.sync.params[self._order[0]] if self.grouped else self.flat)
        return int(st["step"]) if st else 0

    @property
    def skipped_steps(self) -> int:
        """Steps the guard has refused so far.  Reads the device counter on the HIP form: synchronises."""
        if self._hip:
            return int(self._skip_ctr[self._skip_cur]) if self._ex else 0
        return self._skipped

    @property
    def applied_steps(self) -> int:
        """Steps applied so far: Adam's step count.  May synchronise, as skipped_steps."""
        return self._t - self.skipped_steps if self._hip else self._applied_torch()

    # ------------------------------------------------------------------ averaged weights
    def reset_ema(self) -> None:
        """ema <- the current parameters.  Done at construction; with data parallelism call it again after
        ``broadcast_parameters`` so that every rank averages from the same start."""
        if self.ema is None:
            raise RuntimeError("FlatAdam.reset_ema: constructed without ema_decay")
        with torch.no_grad():
            self.ema.copy_(self.flat.data)

    def _swap_ema(self) -> None:
        if self._hip:
            from . import _lib
            from . import functional as F_
            _lib.check(_lib.load().ggpm_flat_swap(F_._p(self.flat.data), F_._p(self.ema), self.flat.numel(), F_._stream()),
                       "flat_swap")
            return
        with torch.no_grad():
            tmp = self.flat.data.clone()
            self.flat.data.copy_(self.ema)
            self.ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights():`` the model's parameters hold the averaged weights (and ``ema`` the trained ones) inside
        the body: the two flat buffers exchange their contents in place, one launch each way, also when the body raises.
        Evaluate, decode or ``model.state_dict()`` inside; do not step."""
        if self.ema is None:
            raise RuntimeError("FlatAdam.ema_weights: constructed without ema_decay")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    # ------------------------------------------------------------------ checkpoints
    def _moments(self):
        """(exp_avg, exp_avg_sq) as parameter-shaped views, one pair of lists in ``sync.params`` order; None before any state."""
        params, offs = self.sync.params, self.sync.offsets
        if self._hip:
            flat_m, flat_v = self._m, self._v
        elif not self.grouped:
            st = self.opt.state.get(self.flat)
            if not st:
                return None
            flat_m, flat_v = st["exp_avg"], st["exp_avg_sq"]
        else:
            sts = [self.opt.state.get(p) for p in params]
            if not all(sts):
                return None
            return [st["exp_avg"] for st in sts], [st["exp_avg_sq"] for st in sts]
        return ([flat_m[o:o + p.numel()].view_as(p) for p, o in zip(params, offs)],
                [flat_v[o:o + p.numel()].view_as(p) for p, o in zip(params, offs)])

    def state_dict(self) -> dict:
        """``torch.optim.Adam(...).state_dict()`` over the individual parameters: ``param_groups`` from ``opt`` with ``params``
        numbered group by group, ``state[i] = {"step", "exp_avg", "exp_avg_sq"}`` (clones, parameter shaped, no padding; empty
        before the first applied step) -- torch's own ``load_state_dict`` takes it.  One more top-level key, ``"flat_adam"``,
        carries ``{"version": 1, "calls", "skipped", "ema", "ema_decay", "ema_warmup"}``: Adam's ``step`` is calls - skipped.
        Synchronises on the HIP form (it reads the skipped-step counter)."""
        skipped = self.skipped_steps
        applied = self.applied_steps
        groups, start = [], 0
        for grp, mine in zip(self.opt.param_groups, self._slots):
            groups.append(dict({k: v for k, v in grp.items() if k != "params"}, params=list(range(start, start + len(mine)))))
            start += len(mine)
        state = {}
        mv = self._moments() if applied > 0 else None
        if mv is not None:
            for j, i in enumerate(self._order):
                state[j] = {"step": torch.tensor(float(applied), dtype=torch.float32),
                            "exp_avg": mv[0][i].detach().clone(), "exp_avg_sq": mv[1][i].detach().clone()}
        ema = None if self.ema is None else {j: self.ema_views[i].detach().clone() for j, i in enumerate(self._order)}
        return {"state": state, "param_groups": groups,
                "flat_adam": {"version": 1, "calls": applied + skipped, "skipped": skipped, "ema": ema,
                              "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup}}

    def load_state_dict(self, sd: dict) -> None:
        """Takes a dict of ``state_dict()`` -- written by either form, grouped or not -- or of a plain ``torch.optim.Adam`` over
        the same parameters in the same groups (then calls = step, skipped = 0).  Restores the hyper-parameters into
        ``param_groups`` (every key the dict carries, ``initial_lr`` included, so a scheduler resumes; not the keys that pick
        torch's implementation), the moments (padding stays zero), the counts and the EMA (reset from the parameters when
        the dict has none).  Without ``skip_nonfinite`` nothing can be skipped later, so the counts are folded: calls = step.

        Raises ValueError, before anything is changed, for another number of groups or parameters, a shape mismatch, parameters
        whose ``step`` values differ (one step count serves all), and an EMA in the dict but none in this optimizer."""
        groups, state, extra = sd["param_groups"], sd["state"], sd.get("flat_adam")
        params = self.sync.params
        if len(groups) != len(self._slots):
            raise ValueError("FlatAdam.load_state_dict: the dict has %d parameter group(s), the optimizer %d"
                             % (len(groups), len(self._slots)))
        for k, (grp, mine) in enumerate(zip(groups, self._slots)):
            if len(grp["params"]) != len(mine):
                raise ValueError("FlatAdam.load_state_dict: group %d holds %d parameter(s) in the dict, %d in the optimizer"
                                 % (k, len(grp["params"]), len(mine)))
            if grp.get("amsgrad") or grp.get("maximize"):
                raise ValueError("FlatAdam.load_state_dict: group %d asks for amsgrad / maximize" % k)
        ids = [pid for grp in groups for pid in grp["params"]]           # position j of this list <-> slot _order[j]
        step = None
        for j, (pid, i) in enumerate(zip(ids, self._order)):
            st = state.get(pid)
            t = float(st["step"]) if st else 0.0
            if step is None:
                step = t
            if t != step or t != int(t) or t < 0:
                raise ValueError("FlatAdam.load_state_dict: parameter %d is at step %r, parameter 0 at %r; one step count "
                                 "serves all" % (j, t, step))
            for key in (("exp_avg", "exp_avg_sq") if st else ()):
                if tuple(st[key].shape) != tuple(params[i].shape):
                    raise ValueError("FlatAdam.load_state_dict: %s of parameter %d has shape %s, the parameter %s"
                                     % (key, j, tuple(st[key].shape), tuple(params[i].shape)))
        step = int(step or 0)
        calls, skipped, ema = step, 0, None
        if extra is not None:
            if extra.get("version") != 1:
                raise ValueError("FlatAdam.load_state_dict: 'flat_adam' version %r, this code reads 1" % (extra.get("version"),))
            calls, skipped, ema = int(extra["calls"]), int(extra["skipped"]), extra.get("ema")
            if calls - skipped != step or skipped < 0:
                raise ValueError("FlatAdam.load_state_dict: calls %d - skipped %d is not the parameters' step %d"
                                 % (calls, skipped, step))
        if ema is not None:
            if self.ema is None:
                raise ValueError("FlatAdam.load_state_dict: the dict carries EMA weights, the optimizer was built without "
                                 "ema_decay")
            for j, i in enumerate(self._order):
                if j not in ema or tuple(ema[j].shape) != tuple(params[i].shape):
                    raise ValueError("FlatAdam.load_state_dict: EMA of parameter %d has shape %s, the parameter %s"
                                     % (j, tuple(ema[j].shape) if j in ema else None, tuple(params[i].shape)))
        if not self.skip_nonfinite:
            calls, skipped = step, 0
        # ---- nothing was changed up to here
        for grp, saved in zip(self.opt.param_groups, groups):
            for k, val in saved.items():
                if k not in _IMPL_KEYS:
                    grp[k] = val
        flat = self.flat.data
        with torch.no_grad():
            m, v = (self._m, self._v) if self._hip else (torch.zeros_like(flat), torch.zeros_like(flat))
            if self._hip:
                m.zero_()
                v.zero_()
            for buf, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
                for pid, i in zip(ids, self._order):
                    if step > 0:
                        off, p = self.sync.offsets[i], params[i]
                        buf[off:off + p.numel()].view_as(p).copy_(state[pid][key])
            if self._hip:
                self._t = calls
                if self._ex:
                    self._skip_ctr.fill_(skipped)
            else:
                self._skipped = skipped
                self.opt.state.clear()
                if step > 0:
                    def count(grp, p):                  # where torch.optim.Adam keeps `step` for this kind of group
                        on_dev = grp.get("fused") or grp.get("capturable")
                        return torch.tensor(float(step), dtype=torch.float32, device=p.device if on_dev else "cpu")
                    if not self.grouped:
                        self.opt.state[self.flat] = {"step": count(self.opt.param_groups[0], flat), "exp_avg": m,
                                                     "exp_avg_sq": v}
                    else:
                        for grp, mine in zip(self.opt.param_groups, self._slots):
                            for i in mine:
                                off, p = self.sync.offsets[i], params[i]
                                self.opt.state[p] = {"step": count(grp, p),
                                                     "exp_avg": m[off:off + p.numel()].view_as(p).clone(),
                                                     "exp_avg_sq": v[off:off + p.numel()].view_as(p).clone()}
            if self.ema is not None:
                if ema is None:
                    self.reset_ema()
                else:
                    for j, i in enumerate(self._order):
                        self.ema_views[i].copy_(ema[j])
