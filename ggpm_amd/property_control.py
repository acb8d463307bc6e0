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

``search`` / ``search_and_decode`` are not the reference's: a search that also stays near the molecule's posterior and where
the prior has mass, from several seeded starts, as one launch (ggpm_latent_search_guided, csrc/latent_search.hip) followed by
the choice of the best start (ggpm_latent_search_select).  The three loops above are unchanged beside it.
"""
from __future__ import annotations

import ctypes
import warnings
from collections import namedtuple

import torch
import torch.nn as nn

from . import functional as F_
from .property import check_envelope

MODES = {"fixed": 0, "soft": 1, "patience": 2}
DONE, CAPPED = 0, 1
MAX_STARTS = F_.LIKELIHOOD_MAX_K            # the starts are log_likelihood's draws

LatentSearchResult = namedtuple("LatentSearchResult", ["latent", "predictions", "best_start", "terms", "all_latents",
                                                       "all_objectives", "all_terms", "steps_taken"])
LatentSearchResult.__doc__ = """What ``search`` returns: device tensors (nothing is synchronised) for K starts, B molecules, latent width L.
  latent         [B, L]     the final latent of each molecule's best start
  predictions    (homo [B], lumo [B])  the heads on ``latent``
  best_start     [B] int32  the start with the smallest objective J; ties to the lowest, a NaN behind every number
  terms          [B, 3]     prop, anchor, prior at ``latent``, unweighted
  all_latents    [K, B, L]  every start's final latent
  all_objectives [K, B]     J = prop + anchor_weight anchor + prior_weight prior
  all_terms      [K, B, 3]
  steps_taken    [K, B] int32  updates made (fewer than ``steps`` where ``delta`` ended the trajectory)"""


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


    def search(self, batch, n_starts=1, steps=None, lr=None, momentum=0.9, anchor_weight=0.0, prior_weight=0.0, prior=None,
               delta=None, weights=(1.0, 1.0), seed=None, sample_ids=None):
        """A regularised, multi-start search (every trajectory and every step in ONE launch,
        csrc/latent_search.hip, the choice of the best start in a second): per molecule ``n_starts`` trajectories of
        gradient descent with heavy-ball ``momentum`` on

            J(v) = w_h (homo(v) - t_h)^2 + w_l (lumo(v) - t_l)^2 + anchor_weight anchor(v) + prior_weight prior(v)

        with anchor(v) = 0.5 sum_j (v_j - mu_j)^2 exp(-lv_j) -- the molecule's posterior, which keeps v near its source --
        and prior(v) = -log p(v) under the standard normal or ``prior`` (a :class:`~ggpm_amd.prior.MixturePrior`); then the
        start with the smallest J.  ``steps`` and ``lr`` default to ``property_optim_step`` and ``lr`` (``latent_lr``);
        ``delta`` (default None: no early exit) ends a trajectory once the property term is <= delta; ``weights`` = (w_h, w_l).

        Starts: the batch is encoded once; start 0 is the posterior mean, start k >= 1 is ``mu + exp(lv / 2) eps_k`` with
        ``eps_k`` draw k of ``log_likelihood(batch, n_samples >= k + 1, seed=seed, sample_ids=sample_ids)`` -- site LATENT of
        the seeded stream, counter ``k * L + column`` --, so ``z[k]`` of that call is start k (its draw 0 is not used here).  A
        molecule's starts depend on ``seed`` (None: from torch's CPU generator) and its sample id only, not on its batch.
        No parameter ``.grad`` is touched and no state is left on the optimizer or the model."""
        from . import _lib
        from .greedy_decode import split_seed
        from .latent_heads import _encode_heads
        from .nnutils import make_cuda
        from .prior import check_prior
        opt = self.model.property_optim
        if opt.training and (opt.homo_linear.dropout > 0 or opt.lumo_linear.dropout > 0):
            raise RuntimeError("latent search: the property heads are in training mode with dropout > 0; call "
                               "model.eval() first (the search runs the heads without dropout)")
        tensors, homos, lumos = batch[2], batch[4], batch[5]
        half = opt.input_size
        L, B = 2 * half, len(homos)
        if isinstance(n_starts, bool) or int(n_starts) != n_starts or not 1 <= int(n_starts) <= MAX_STARTS:
            raise ValueError("latent search: n_starts %r (1 .. %d)" % (n_starts, MAX_STARTS))
        K = int(n_starts)
        steps = int(self.property_optim_step if steps is None else steps)
        lr = float(self.lr if lr is None else lr)
        w_h, w_l = (float(w) for w in weights)
        values = dict(steps=steps, momentum=float(momentum), anchor_weight=float(anchor_weight),
                      prior_weight=float(prior_weight), w_homo=w_h, w_lumo=w_l)
        for what, v in values.items():
            if not 0 <= v < float("inf"):
                raise ValueError("latent search: %s %r (a finite value >= 0)" % (what, v))
        if sample_ids is not None and len(sample_ids) != B:
            raise ValueError("latent search: %d sample_ids for %d molecules" % (len(sample_ids), B))
        dev = self.model.R_mean.weight.device
        prior = check_prior("latent search", prior, L, dev)
        check_envelope(opt, 1)
        with torch.no_grad():
            _, mu, pre_var = _encode_heads(self.model, make_cuda(tensors))
            if mu.dtype != torch.float32:
                raise NotImplementedError("latent search: fp32 latents only")
            if mu.shape != (B, L):
                raise ValueError("latent search: %d targets, a latent of %s" % (B, tuple(mu.shape)))
            t = [torch.as_tensor(x, dtype=torch.float32).to(dev).reshape(-1).contiguous() for x in (homos, lumos)]
            if t[1].numel() != B:
                raise ValueError("latent search: %d rows, targets of %d / %d" % (B, t[0].numel(), t[1].numel()))
            mu, lv = mu.contiguous(), -pre_var.abs()
            if K == 1:
                z0 = mu.reshape(1, B, L)
            else:
                lo, hi = split_seed(seed)
                z0 = F_.latent_terms(mu, pre_var, F_.sample_latent_normal(K, B, L, lo, hi, ids=sample_ids, device=dev))[0]
                z0[0] = mu
            f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
            z_all, pred_all = torch.empty(K, B, L, **f32), torch.empty(2, K * B, **f32)
            terms_all, J, n = torch.empty(K, B, 3, **f32), torch.empty(K, B, **f32), torch.empty(K, B, **i32)
            heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
            mix = (None, None, None) if prior is None else tuple(
                p.detach().contiguous() for p in (prior.logits, prior.means, prior.log_vars))
            lib = _lib.load()
            _lib.check(lib.ggpm_latent_search_guided(
                K, B, F_._p(z0), L, half, F_._p(mu), F_._p(lv), ctypes.byref(heads[0]), ctypes.byref(heads[1]), F_._p(t[0]),
                F_._p(t[1]), F_._p(mix[0]), F_._p(mix[1]), F_._p(mix[2]), 0 if prior is None else prior.n_components, lr,
                values["momentum"], steps, -1.0 if delta is None else float(delta), w_h, w_l, values["anchor_weight"],
                values["prior_weight"], F_._p(z_all), F_._p(pred_all), F_._p(terms_all), F_._p(J), F_._p(n), F_._stream()),
                "latent_search_guided")
            best, latent = torch.empty(B, **i32), torch.empty(B, L, **f32)
            pred, terms = torch.empty(2, B, **f32), torch.empty(B, 3, **f32)
            _lib.check(lib.ggpm_latent_search_select(F_._p(J), F_._p(z_all), F_._p(pred_all), F_._p(terms_all), K, B, L,
                                                     F_._p(best), F_._p(latent), F_._p(pred), F_._p(terms), F_._stream()),
                       "latent_search_select")
        return LatentSearchResult(latent, (pred[0], pred[1]), best, terms, z_all, J, terms_all, n)

    def search_and_decode(self, batch, args=None, **search_kwargs):
        """``search(batch, **search_kwargs)``, then the decoder's greedy ``decode`` of 150 steps on the selected latent, as
        ``forward`` decodes its own -> ((homo [B], lumo [B]), (results, molecules))."""
        from .property_vae import _graph_batch_factory
        factory = _graph_batch_factory(self.model, args)
        res = self.search(batch, **search_kwargs)
        latent = res.latent
        return res.predictions, self.model.decoder.decode(batch[0], (latent, latent, latent), greedy=True,
                                                          max_decode_step=150, graph_batch_factory=factory)


class HierPropertyVAEOptimizer(PropertyVAEOptimizer):
    """The search over HierPropOptVAE's latent (reference ggpm/property_control.py:183-213)."""
