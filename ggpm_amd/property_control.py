"""Latent property search -- reference ggpm/property_control.py (PropertyVAEOptimizer, HierPropertyVAEOptimizer).

Each of ``hard_optimize`` (``fixed``), ``soft_optimize`` and ``patience_optimize`` is ONE library call
(ggpm_property_latent_search, csrc/property.hip): one workgroup per molecule runs its whole trajectory -- forward of both
heads, gradient with respect to the latent, the stopping rule, the reference's signed update -- with the heads' weights in
LDS.  The reference loops in Python per molecule and reads the loss back to the host two or three times per step.

Differences from the reference, on purpose:
  * the loop is bounded: ``max_steps`` (args.max_steps, default 10000) loop bodies per molecule at most.  The
    reference's soft / patience loops need not end (a loss of exactly 0 makes |0 - 0| / 0 NaN, and the patience is
    reset on every step); a molecule that reaches the bound ends ``capped`` and a warning names how many did;
  * parameter ``.grad``s are left untouched: the reference's per-step ``model.zero_grad()`` (which clears every
    parameter gradient of the model as a side effect) is not reproduced;
  * the heads must be in eval form (``model.eval()``, as optimize.py runs) or have dropout 0: the search applies no
    dropout, so heads in training mode with dropout > 0 raise.
``forward`` ends, as the reference's does, in the decoder's greedy ``decode`` (``MotifDecoder.decode`` for the tree-only
PropOptVAE, ``HierMPNDecoder.decode`` for HierPropOptVAE) through the graph batch ``args.graph_batch_factory`` (else the
decoder's).  ``optimize(batch)`` returns everything before the decode.
"""
from __future__ import annotations

import ctypes
import warnings

import torch
import torch.nn as nn

from . import functional as F_
from .property import check_envelope

MODES = {"fixed": 0, "soft": 1, "patience": 2}
DONE, CAPPED = 0, 1


class PropertyVAEOptimizer(nn.Module):
    """Same constructor and attributes as the reference (``property_optim_step``, ``patience``, ``optimize_type``,
    ``property_delta``, ``patience_threshold``, ``lr``) plus ``max_steps``.  After a search, ``steps_taken`` and
    ``status`` (int32 [B] on the device: loop bodies executed; 0 done, 1 capped) describe it."""

    def __init__(self, model, args):
        super().__init__()
        self.model = model
        self.property_optim_step = args.property_optim_step
        self.patience = args.patience
        self.optimize_type = args.optimize_type
        self.property_delta = args.property_delta
        self.patience_threshold = args.patience_threshold
        self.lr = args.latent_lr
        self.max_steps = int(getattr(args, "max_steps", 10000))
        self.func_dict = {'fixed': self.hard_optimize, 'patience': self.patience_optimize, 'soft': self.soft_optimize}
        self.steps_taken = self.status = None

    def _get_optimize_func(self):
        if self.optimize_type not in self.func_dict:
            raise ValueError("Error: property-optimizing choice \"{}\" is not valid".format(self.optimize_type))
        return self.func_dict[self.optimize_type]

    def forward(self, batch, args=None):
        """reference ggpm/property_control.py:33-63 (the tree-only PropOptVAE) and :186-216 (HierPropOptVAE):
        ``optimize(batch)``, the heads on the optimised latent, greedy decode of 150 steps -> ((homo [B], lumo [B]),
        (results, molecules))."""
        from .property_vae import _graph_batch_factory
        dec = self.model.decoder
        factory = _graph_batch_factory(self.model, args)
        latent, _ = self.optimize(batch)
        half = self.model.latent_size
        with torch.no_grad():
            props = self.model.property_optim.predict(homo_vecs=latent[:, :half], lumo_vecs=latent[:, half:])
        return props, dec.decode(batch[0], (latent, latent, latent), greedy=True, max_decode_step=150,
                                 graph_batch_factory=factory)

    def _search(self, mode, homo_vecs, lumo_vecs, homo_targets, lumo_targets):
        from . import _lib
        opt = self.model.property_optim
        if opt.training and (opt.homo_linear.dropout > 0 or opt.lumo_linear.dropout > 0):
            raise RuntimeError("latent search: the property heads are in training mode with dropout > 0; call "
                               "model.eval() first (the search runs the heads without dropout)")
        half = opt.input_size
        with torch.no_grad():
            z = torch.cat([homo_vecs.detach().reshape(-1, half), lumo_vecs.detach().reshape(-1, half)], dim=-1)
            F_._need_gpu(z)
            if z.dtype != torch.float32:
                raise NotImplementedError("latent search: fp32 latents only")
            z = z.contiguous()
            B = z.shape[0]
            check_envelope(opt, 1)
            t = [torch.as_tensor(x, dtype=torch.float32).to(z.device).reshape(-1).contiguous()
                 for x in (homo_targets, lumo_targets)]
            if t[0].numel() != B or t[1].numel() != B:
                raise ValueError("latent search: %d rows, targets of %d / %d" % (B, t[0].numel(), t[1].numel()))
            z_out = torch.empty_like(z)
            pred = torch.empty(2, B, dtype=torch.float32, device=z.device)
            steps = torch.empty(B, dtype=torch.int32, device=z.device)
            status = torch.empty(B, dtype=torch.int32, device=z.device)
            heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
            _lib.check(_lib.load().ggpm_property_latent_search(
                MODES[mode], B, F_._p(z), z.shape[1], half, ctypes.byref(heads[0]), ctypes.byref(heads[1]), F_._p(t[0]),
                F_._p(t[1]), float(self.lr), int(self.property_optim_step), float(self.property_delta),
                float(self.patience), float(self.patience_threshold), self.max_steps, F_._p(z_out), F_._p(pred),
                F_._p(steps), F_._p(status), F_._stream()), "property_latent_search")
        self.steps_taken, self.status, self.predictions = steps, status, (pred[0], pred[1])
        n_capped = int((status == CAPPED).sum())
        if n_capped:
            warnings.warn("latent search (%s): %d of %d molecules reached max_steps=%d without meeting the stopping rule"
                          % (mode, n_capped, B, self.max_steps), RuntimeWarning)
        return z_out

    def soft_optimize(self, homo_vecs, lumo_vecs, homo_targets, lumo_targets):
        return self._search("soft", homo_vecs, lumo_vecs, homo_targets, lumo_targets)

    def patience_optimize(self, homo_vecs, lumo_vecs, homo_targets, lumo_targets):
        return self._search("patience", homo_vecs, lumo_vecs, homo_targets, lumo_targets)

    def hard_optimize(self, homo_vecs, lumo_vecs, homo_targets, lumo_targets):
        return self._search("fixed", homo_vecs, lumo_vecs, homo_targets, lumo_targets)

    def optimize(self, batch):
        """Everything the reference's ``forward`` does before ``decode`` (ggpm/property_control.py:33-60 for the tree-only
        PropOptVAE, :183-213 for HierPropOptVAE): encode, rsample without noise, the search (``optimize_type``), the heads
        on the final latent.  -> (latent [B, 2 half], (homo_pred [B], lumo_pred [B])); ``steps_taken`` / ``status`` hold
        the per-molecule step counts and outcomes."""
        _, _, tensors, _, homos, lumos = batch
        with torch.no_grad():
            root_vecs, _ = self.model.encode_latent(tensors, perturb=False)
        half = self.model.latent_size
        latent = self._get_optimize_func()(homo_vecs=root_vecs[:, :half], lumo_vecs=root_vecs[:, half:],
                                           homo_targets=homos, lumo_targets=lumos)
        return latent, self.predictions


class HierPropertyVAEOptimizer(PropertyVAEOptimizer):
    """The search over HierPropOptVAE's latent (reference ggpm/property_control.py:183-213)."""
