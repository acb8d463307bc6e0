"""The models of the reference's ggpm/property_vae.py: HierPropertyVAE, HierPropOptVAE, PropertyVAE and PropOptVAE -- encoder,
latent heads, teacher-forced decoder, for the -opt models the property heads -- on one base (``_VAE``), and the encoder-only
HierEncoderVAE.  The latent heads and ``rsample`` are in latent_heads.py; ``log_likelihood``, ``bound_loss``, the latent
accumulators and their result types are in objectives.py and importable from here as before.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _dev
from . import functional as F_
from .decoder_heads import check_no_dropout
from .encoder import HierMPNEncoder
from .latent_heads import _KLHead, _LatentTerms, _latent_heads, rsample  # noqa: F401  (the last three: importable from here)
from .nnutils import make_cuda
from .objectives import (ESTIMATORS, DecompositionObjective, EstimatorObjective, FreeBitsObjective,  # noqa: F401
                         LatentAccumulator, LatentDecomposition, LatentDecompositionAccumulator, LatentStats, MolLikelihood,
                         MolObjective, PriorEstimatorObjective, PriorLikelihood, PriorObjective, bound_loss, log_likelihood)
from .prior import MixturePrior, check_prior  # noqa: F401


class HierEncoderVAE(nn.Module):
    """``encoder`` / ``R_mean`` / ``R_var`` exactly as HierPropertyVAE names them (state_dict compatible)."""

    def __init__(self, args):
        super().__init__()
        self.encoder = HierMPNEncoder(args.vocab, args.atom_vocab, args.rnn_type, args.embed_size, args.hidden_size,
                                      args.depthT, args.depthG, args.dropout)
        self.latent_size = args.latent_size
        self.R_mean = nn.Linear(args.hidden_size, args.latent_size)
        self.R_var = nn.Linear(args.hidden_size, args.latent_size)

    def forward(self, tensors, beta=0.0, perturb_z=True, prep=None, beside=False):
        tree_tensors, graph_tensors = make_cuda(tensors)
        hroot, hnode, hinter, hatom = self.encoder.forward_padded(tree_tensors, graph_tensors, prep, beside=beside)
        z, kl = rsample(hroot, self.R_mean, self.R_var, perturb_z)
        H = self.encoder.hidden_size
        return z, kl, (hroot[:, :H], hnode[:, :H], hinter[:, :H], hatom[:, :H])


class StepMetrics(dict):
    """The metrics dictionary ``HierPropertyVAE.forward`` returns (ggpm/property_vae.py:60-62 builds it with ``.item()``:
    python floats).  Same keys, same values -- read on FIRST ACCESS: the six device scalars are stacked by one kernel when
    the forward ends, their copy into pinned host memory is enqueued right behind it, and a value is taken from there
    when it is asked for, which in ``vae_train.py`` is after ``loss.backward(); optimizer.step()`` (:81-86).  Reading them
    inside the forward, as the reference does, stops the host in the middle of the step: the backward cannot be issued
    while the forward's tail still runs.  The read waits for the copy's event, not for the stream: like the reference's
    loop, the host goes on to the next batch while the GPU still finishes this step's backward and optimizer."""

    _KEYS = ('Loss', 'KL:', 'Word', 'I-Word', 'Topo', 'Assm')

    def __init__(self, values):
        super().__init__()
        vals = [v.detach().reshape(()).float() if isinstance(v, torch.Tensor) else None for v in values]
        self._const = [None if isinstance(v, torch.Tensor) else float(v) for v in values]
        dev = next((v.device for v in vals if v is not None), None)
        self._dev = torch.stack([v if v is not None else torch.zeros((), device=dev) for v in vals]) if dev is not None else None
        self._ready = False
        self._host = self._event = None
        if self._dev is not None and self._dev.is_cuda and _dev.METRICS_ASYNC:
            # the copy to the host is ENQUEUED here, behind the forward; a reader waits for this event only -- not for
            # whatever the stream has been given since (backward, optimizer), so the loop can go on to the next batch
            # while the step's tail still runs, as it does around the reference's .item() calls
            self._host = torch.empty(len(self._KEYS), dtype=torch.float32, pin_memory=True)
            self._host.copy_(self._dev, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()

    def _fill(self):
        if not self._ready:
            if self._event is not None:
                self._event.synchronize()
                host = self._host.tolist()
            else:
                host = self._dev.tolist() if self._dev is not None else [0.0] * len(self._KEYS)
            for k, h, c in zip(self._KEYS, host, self._const):
                dict.__setitem__(self, k, h if c is None else c)
            self._ready = True

    def __getitem__(self, k):
        self._fill()
        return dict.__getitem__(self, k)

    def __iter__(self):
        return iter(self._KEYS)

    def __len__(self):
        return len(self._KEYS)

    def __contains__(self, k):
        return k in self._KEYS

    def keys(self):
        return list(self._KEYS)

    def values(self):
        self._fill()
        return [dict.__getitem__(self, k) for k in self._KEYS]

    def items(self):
        self._fill()
        return [(k, dict.__getitem__(self, k)) for k in self._KEYS]

    def get(self, k, default=None):
        return self[k] if k in self._KEYS else default

    def __repr__(self):
        self._fill()
        return dict.__repr__(self)


class PropStepMetrics(StepMetrics):
    """The metrics dictionary of ``HierPropOptVAE.forward`` (ggpm/property_vae.py:249-252), read lazily like StepMetrics
    (values are taken as fp32 on the device, python floats when read)."""

    _KEYS = ('Loss', 'KL', 'Recs_Loss', 'HOMO_MSE', 'LUMO_MSE', 'Word', 'I-Word', 'Topo', 'Assm')


def _eager_metrics() -> bool:
    """Whether this call reads its metrics inside the forward, as the reference does (read at call time)."""
    return os.environ.get("GGPM_LAZY_METRICS", "1") == "0"


def _metrics(cls, values):
    """The metrics of one step under ``cls._KEYS``: ``cls(values)``, read on first access (StepMetrics), or in the eager form
    the reference's dictionary of python floats (``.item()`` inside the forward)."""
    if _eager_metrics():
        return {k: v.item() if isinstance(v, torch.Tensor) else float(v) for k, v in zip(cls._KEYS, values)}
    return cls(values)


class LossClipped:
    """The third value of ``HierPropOptVAE.forward``: whether ``clip_negative_loss`` replaced the loss.  The decision
    stays on the device; ``bool()`` reads it (vae_fine_tune.py reads it after ``optimizer.step()``)."""

    def __init__(self, flag):
        self._flag = flag

    def __bool__(self):
        if isinstance(self._flag, torch.Tensor):
            self._flag = bool(self._flag.item())
        return bool(self._flag)

    def __repr__(self):
        return repr(bool(self))


class _ClipNegativeLoss:
    """``clip_negative_loss`` of the reference's two property-optimising models (HierPropOptVAE, PropOptVAE): a total that
    is not > 0 is replaced by a draw of N(0.5, 0.5) from ``clip_generator`` (see HierPropOptVAE)."""

    @property
    def clip_generator(self) -> torch.Generator:
        """The generator of clip_negative_loss's replacement draws (created on the model's device, seeded with
        ``torch.initial_seed()``; reseed it with ``manual_seed`` for a repeatable run)."""
        dev = self.R_mean.weight.device
        if self._clip_gen is None or self._clip_gen.device != dev:
            self._clip_gen = torch.Generator(device=dev)
            self._clip_gen.manual_seed(torch.initial_seed())
        return self._clip_gen

    def clip_negative_loss(self, loss):
        noise = lambda: torch.normal(mean=0.5, std=0.5, size=loss.size(), dtype=loss.dtype, device=loss.device,  # noqa
                                     generator=self.clip_generator)
        if _eager_metrics():
            if loss > 0:
                return False, loss
            return True, loss * 0 + noise()
        clipped = torch.logical_not(loss > 0)            # NaN counts as clipped, as `if loss > 0` does
        return LossClipped(clipped.reshape(-1)[0]), torch.where(clipped, loss * 0 + noise(), loss)


class _VAE(nn.Module):
    """What the four models share: the sub-modules, the encode step, the decoder's bookkeeping, the forward of the two
    models without property heads, and the methods that differ in nothing but the model they are called on."""

    HIER = True                 # encoder(tree_tensors, graph_tensors) and a decoder with an atom level; False: tree-only
    PROPERTY_HEADS = False      # the HOMO / LUMO heads on the two latent halves (the -opt models)

    def _build(self, args, encoder_cls, decoder_cls, tie_always=False):
        """The sub-modules, in the order that fixes the state_dict, ``parameters()`` (FlatAdam's flat buffer, bound_loss's
        parameter tuple) and the draws of the initial weights: encoder, decoder, [property_optim], R_mean, R_var,
        [loss_weigh].  Tying draws nothing and registers nothing on the model, so where it stands among them shows nowhere."""
        heads = self.PROPERTY_HEADS
        if heads and args.latent_size % 2 != 0:
            raise ValueError("%s: latent_size must be even (the HOMO and LUMO heads read one half each), got %d"
                             % (type(self).__name__, args.latent_size))
        self.encoder = encoder_cls(args.vocab, args.atom_vocab, args.rnn_type, args.embed_size, args.hidden_size,
                                   args.depthT, args.depthG, args.dropout)
        self.decoder = decoder_cls(args.vocab, args.atom_vocab, args.rnn_type, args.embed_size, args.hidden_size,
                                   args.latent_size, args.diterT, args.diterG, args.dropout)
        if tie_always or getattr(args, "tie_embedding", False):
            self.encoder.tie_embedding(self.decoder.hmpn)
        self.latent_size = args.latent_size // 2 if heads else args.latent_size
        if heads:
            from .property import LossWeigh, PropertyOptimizer
            self.property_optim = PropertyOptimizer(input_size=self.latent_size, hidden_size=args.linear_hidden_size,
                                                    dropout=args.dropout)
            self.property_optim_step = args.property_optim_step
        self.R_mean = nn.Linear(args.hidden_size, args.latent_size)
        self.R_var = nn.Linear(args.hidden_size, args.latent_size)
        if heads:
            self.loss_scaling = bool(getattr(args, "loss_scaling", False))
            if self.loss_scaling:
                self.loss_weigh = LossWeigh()
            self._clip_gen = None

    def _decode_schedule(self, graphs, tensors, orders, schedule):
        """The decoder's bookkeeping: the one passed, the one ScheduleAhead attached to ``graphs`` (built one batch ahead),
        or derived here."""
        if schedule is None:
            schedule = getattr(graphs, "ggpm_schedule", None)
        if schedule is None and graphs is not None:
            # the reference's call shape, ``model(*batch, beta=beta)`` (vae_train.py:78): derive the decoder's integer
            # bookkeeping HERE, from the batch as it arrives (host arrays: no read-back), so that the atom level can be
            # issued beside the encoder exactly as with a prepared schedule
            from .decoder import DecodeSchedule
            schedule = DecodeSchedule.from_graphs(graphs, tensors, orders, self.decoder.vocab, **self.decoder.schedule_hints())
        return schedule

    def _encode(self, tensors):
        """The encoder's root vectors of ``tensors`` (on the device)."""
        tree_tensors, graph_tensors = tensors
        if not self.HIER:
            return self.encoder.forward_padded(tree_tensors)[0]
        return self.encoder.forward_padded(tree_tensors, graph_tensors)[0]

    def _encode_beside_atom_level(self, tensors, schedule):
        """The training forwards' encoder call -> (root vectors, what the decoder's call takes besides: ``atom=``, the
        handle of its atom level).  The hierarchical decoder's atom level of ``schedule`` does not depend on the latent
        vector: it is posted first and issued beside the encoder.  (A tree-only decoder has no atom level.)"""
        if not self.HIER:
            return self._encode(tensors), {}
        F_.mark("fwd: inputs on the device")
        atom = self.decoder.start_atom_level(schedule, tensors)
        F_.mark("fwd: atom level posted")
        # beside the atom level's chain of small launches the encoder's levels take half as many (twice as large)
        # workgroups: the chain's launches then find free compute units instead of waiting for the encoder's to drain
        return self.encoder.forward_padded(*tensors, beside=atom is not None)[0], dict(atom=atom)

    def forward(self, mols, graphs, tensors, orders, homos=None, lumos=None, beta=0.0, perturb_z=True, schedule=None):
        schedule = self._decode_schedule(graphs, tensors, orders, schedule)
        tensors = make_cuda(tensors)
        root_vecs, ahead = self._encode_beside_atom_level(tensors, schedule)
        root_vecs, kl_div = rsample(root_vecs, self.R_mean, self.R_var, perturb_z)
        F_.mark("fwd: encoder + rsample issued")
        loss, wacc, iacc, tacc, sacc = self.decoder(mols, (root_vecs, root_vecs, root_vecs), graphs, tensors, orders,
                                                    schedule=schedule, **ahead)
        loss = loss + beta * kl_div
        F_.mark("fwd: heads and losses issued")
        return loss, _metrics(StepMetrics, (loss, kl_div, wacc, iacc, tacc, sacc))

    def rsample(self, z_vecs, perturb=True):
        return rsample(z_vecs, self.R_mean, self.R_var, perturb)

    def sample(self, batch_size, greedy=True, seed=None, max_decode_step=150, beam=5, graph_batch_factory=None, prior=None):
        """New molecules from the prior (what reference ggpm/property_vae.py:35-37 intends): seeded standard-normal latents
        drawn on the device -- with ``prior`` (a :class:`MixturePrior`) its ``sample(batch_size, seed=seed)`` instead --,
        then ``decode`` or, with ``greedy=False``, ``decode_sampled`` at the same seed -> (results, molecules)."""
        return _sample(self, batch_size, greedy, seed, max_decode_step, beam, graph_batch_factory, prior)

    def log_likelihood(self, batch, n_samples=1, seed=None, sample_ids=None, eps=None, max_cls_size=None, schedule=None,
                       prior=None):
        """Per-molecule reconstruction terms, KL, ELBO and the ``n_samples``-sample importance-weighted bound of ``batch``
        (the tuple ``self(*batch)`` takes), under the standard normal or ``prior`` -> :class:`MolLikelihood`; forward only,
        see :func:`log_likelihood`."""
        return log_likelihood(self, batch, n_samples, seed, sample_ids, eps, max_cls_size, schedule, prior)

    def bound_loss(self, batch, n_samples=1, objective="elbo", beta=1.0, mol_weights=None, seed=None, sample_ids=None,
                   eps=None, max_cls_size=None, schedule=None, estimator="reparam", prior=None, alpha=None, gamma=None,
                   dataset_size=None, free_bits=None):
        """The ``n_samples``-sample ELBO (``objective="elbo"``), importance-weighted bound (``"iwae"``) or beta-TCVAE loss
        (``"tcvae"``, with ``alpha``, ``gamma`` and ``dataset_size``) of ``batch`` as a loss to train on, with optional
        per-molecule weights, for the ELBO a free-bits KL and for the importance-weighted bound a choice of gradient
        estimator, and for the ELBO and the importance-weighted bound a learned ``prior`` -> (loss, :class:`MolObjective`);
        see :func:`bound_loss`."""
        return bound_loss(self, batch, n_samples, objective, beta, mol_weights, seed, sample_ids, eps, max_cls_size, schedule,
                          estimator, prior, alpha, gamma, dataset_size, free_bits)

    def latent_decomposition_accumulator(self, dataset_size, n_samples=1, seed=None):
        """A :class:`LatentDecompositionAccumulator` of this model: the split of the KL into mutual information, total
        correlation and dimension-wise KL over as many batches as it is given, kept on the device."""
        return LatentDecompositionAccumulator(self, dataset_size, n_samples, seed)

    def latent_decomposition(self, batches, dataset_size, n_samples=1, seed=None):
        """The index-code mutual information, the total correlation and the dimension-wise KL (in all and per column) of
        the latent over the iterable ``batches``, every batch estimating q(z) by minibatch-weighted sampling from its own
        molecules and ``dataset_size`` -> :class:`LatentDecomposition`."""
        acc = self.latent_decomposition_accumulator(dataset_size, n_samples, seed)
        for batch in batches:
            acc.update(batch)
        return acc.result()

    def latent_accumulator(self, au_threshold=0.01):
        """A :class:`LatentAccumulator` of this model: per-dimension statistics of the latent over as many batches as it is
        given, kept on the device."""
        return LatentAccumulator(self, au_threshold)

    def latent_stats(self, batches, au_threshold=0.01):
        """Per-dimension KL, the mean and variance of the posterior means, the mean posterior variance and the number of
        active units (``Var_x E_q[z_j] > au_threshold``) over the iterable ``batches`` -> :class:`LatentStats`."""
        acc = self.latent_accumulator(au_threshold)
        for batch in batches:
            acc.update(batch)
        return acc.result()

    def reconstruct(self, batch, args=None):
        """reference ggpm/property_vae.py:39-45 (101-109, 169-188, 299-318 for the other three): the no-grad encoder, the
        mean latent, for the -opt models the property heads on it, greedy decode of 150 steps -> (results, molecules), for
        the -opt models ((homo [B], lumo [B]), (results, molecules)).  The graph batch: ``args.graph_batch_factory``, else
        the decoder's."""
        factory = _graph_batch_factory(self, args)
        with torch.no_grad():
            root_vecs, _ = rsample(self._encode(make_cuda(batch[2])), self.R_mean, self.R_var, perturb=False)
            props = self._property_heads(root_vecs) if self.PROPERTY_HEADS else None
        decoded = self.decoder.decode(batch[0], (root_vecs, root_vecs, root_vecs), greedy=True, max_decode_step=150,
                                      graph_batch_factory=factory)
        return (props, decoded) if self.PROPERTY_HEADS else decoded


class _PropOptVAE(_ClipNegativeLoss, _VAE):
    """The two property-optimising models: the heads on the two latent halves and the forward with their losses."""

    PROPERTY_HEADS = True
    KL_IN_LOSS = False          # whether ``beta * KL`` joins the reconstruction loss (before ``loss_scaling``)

    def _property_heads(self, z):
        half = self.latent_size
        return self.property_optim.predict(homo_vecs=z[:, :half], lumo_vecs=z[:, half:])

    def encode_latent(self, tensors, perturb=False):
        """Encoder + rsample of the reference's search (ggpm/property_control.py:194-200): -> (latent [B, 2 half], kl)."""
        return rsample(self._encode(make_cuda(tensors)), self.R_mean, self.R_var, perturb)

    def predict_properties(self, batch):
        """The property predictions the reference's ``reconstruct`` forms before it decodes (ggpm/property_vae.py:169-186):
        encoder, the mean latent (no noise), both heads -- under no-grad, so every stage runs its forward-only form.
        ``batch`` is a reference batch (mols, graphs, tensors, orders, homos, lumos).  -> (homo [B], lumo [B])."""
        with torch.no_grad():
            return self._property_heads(self.encode_latent(batch[2], perturb=False)[0])

    def forward(self, mols, graphs, tensors, orders, homos, lumos, beta=0.0, perturb_z=True, schedule=None):
        schedule = self._decode_schedule(graphs, tensors, orders, schedule)
        tensors = make_cuda(tensors)
        root_vecs, ahead = self._encode_beside_atom_level(tensors, schedule)
        if perturb_z or self.KL_IN_LOSS:
            root_vecs, kl_div = rsample(root_vecs, self.R_mean, self.R_var, perturb_z)
        else:
            # z = mean: KL is a metric only, so R_var stays out of the graph (its .grad stays None, as in the reference)
            root_vecs, kl_div = _KLHead.apply(root_vecs, self.R_mean.weight, self.R_mean.bias,
                                              self.R_var.weight.detach(), self.R_var.bias.detach(), None)
        dev = root_vecs.device
        t_homo = torch.as_tensor(homos, dtype=torch.float32).to(dev, non_blocking=True)
        t_lumo = torch.as_tensor(lumos, dtype=torch.float32).to(dev, non_blocking=True)
        homo_loss, lumo_loss, _, _ = self.property_optim.forward_latent(root_vecs, (t_homo, t_lumo))
        loss, wacc, iacc, tacc, sacc = self.decoder(mols, (root_vecs, root_vecs, root_vecs), graphs, tensors, orders,
                                                    schedule=schedule, **ahead)
        if self.KL_IN_LOSS:
            loss = loss + beta * kl_div
        if self.loss_scaling:
            loss = self.loss_weigh.compute_recon_loss(loss)
            homo_loss, lumo_loss = self.loss_weigh.compute_prop_loss(homo_loss, lumo_loss)
        total_loss = loss + homo_loss + lumo_loss
        clipped, total_loss = self.clip_negative_loss(total_loss)
        return total_loss, _metrics(PropStepMetrics, (total_loss, kl_div, loss, homo_loss, lumo_loss, wacc, iacc, tacc, sacc)), \
            clipped


class HierPropertyVAE(_VAE):
    """reference ggpm/property_vae.py:11-62 -- encoder, latent heads, teacher-forced decoder; the class
    ``OPVNet.get_model('hier-prop')`` returns (ggpm/opvnet.py:4-9) and ``vae_train.py:78`` calls as
    ``model(*batch, beta=beta)``.  Same constructor argument bag, sub-module names and ``state_dict`` keys.

    ``forward(mols, graphs, tensors, orders, homos, lumos, beta, perturb_z=True)`` returns ``(loss, metrics)`` like the
    reference; ``schedule=`` optionally passes a prepared :class:`ggpm_amd.decoder.DecodeSchedule` (the decoder's
    integer bookkeeping, otherwise derived from ``graphs`` on every call).
    """

    def __init__(self, args):
        super().__init__()
        from .decoder import HierMPNDecoder
        self._build(args, HierMPNEncoder, HierMPNDecoder)

    def rsample(self, z_vecs, W_mean, W_var, perturb=True):
        return rsample(z_vecs, W_mean, W_var, perturb)


class HierPropOptVAE(_PropOptVAE):
    """reference ggpm/property_vae.py:130-254 -- HierPropertyVAE's encoder, rsample and teacher-forced decoder plus the
    HOMO / LUMO heads on the two latent halves (``property_optim``, ggpm_amd.property) and optionally ``LossWeigh``; the
    class ``OPVNet.get_model('hier-prop-opt')`` returns and ``vae_fine_tune.py`` trains.  Same argument bag (plus
    ``linear_hidden_size``, ``property_optim_step``, optional ``loss_scaling``), sub-module names and ``state_dict`` keys.

    ``forward(mols, graphs, tensors, orders, homos, lumos, beta, perturb_z=True, schedule=None)`` ->
    ``(total_loss, metrics, clipped)`` with the reference's arithmetic:
      * total = recon + homo_mse + lumo_mse.  There is NO KL term (the reference's ``loss += beta * kl_div`` sits in a
        string literal): ``beta`` is unused and KL is a metric only.  With ``perturb_z=False`` R_var then receives no
        gradient at all (``.grad`` stays None, as in the reference).
      * ``loss_scaling``: LossWeigh's fp64 weights, as in the reference (the total is then fp64 of shape [1]).
      * ``clip_negative_loss``: a total that is not > 0 is replaced by a draw of N(0.5, 0.5) (gradients then zero).  The
        draw comes from a generator owned by the model (``clip_generator``), so the forward never advances torch's
        global random streams.  By default the decision stays on the device (``torch.where``) and ``clipped`` is a
        ``LossClipped`` whose ``bool()`` reads it; ``GGPM_LAZY_METRICS=0`` uses the reference's host-side form.
    """

    def __init__(self, args):
        super().__init__()
        from .decoder import HierMPNDecoder
        self._build(args, HierMPNEncoder, HierMPNDecoder)


def _sample(model, batch_size, greedy, seed, max_decode_step, beam, graph_batch_factory, prior=None):
    """``sample`` of the four VAEs: [batch_size, decoder.latent_size] latents -- the width ``reconstruct`` hands to
    ``decode`` -- from ``functional.sample_normal`` or, with a prior, from its ``sample`` (sample ids ``arange``), used as all
    three source vectors."""
    from .greedy_decode import split_seed
    dec = model.decoder
    dev = next(dec.parameters()).device
    prior = check_prior("%s.sample" % type(model).__name__, prior, dec.latent_size, dev)
    factory = graph_batch_factory
    if factory is None:
        factory = _graph_batch_factory(model, getattr(model, "args", None))
    check_no_dropout(dec, "%s.sample runs without dropout: call model.eval() first" % type(model).__name__)
    if int(batch_size) < 1:
        raise ValueError("%s.sample: batch_size %d" % (type(model).__name__, batch_size))
    lo, hi = split_seed(seed)
    with torch.no_grad():
        z = F_.sample_normal(int(batch_size), dec.latent_size, lo, hi, device=dev) if prior is None else \
            prior.sample(int(batch_size), seed=lo | hi << 32)
        if greedy:
            return dec.decode(None, (z, z, z), greedy=True, max_decode_step=max_decode_step, beam=beam,
                              graph_batch_factory=factory)
        return dec.decode_sampled(None, (z, z, z), seed=lo | hi << 32, max_decode_step=max_decode_step, beam=beam,
                                  graph_batch_factory=factory)


def _graph_batch_factory(model, args):
    """decode's graph batch for reconstruct: ``args.graph_batch_factory``, else the decoder's; neither raises before the
    batch is touched."""
    factory = getattr(args, "graph_batch_factory", None)
    if factory is None:
        factory = getattr(model.decoder, "graph_batch_factory", None)
    if factory is None:
        raise NotImplementedError(model.decoder.decode_backend().NO_FACTORY)
    return factory


class PropertyVAE(_VAE):
    """reference ggpm/property_vae.py:64-127 -- the tree-only model ``OPVNet.get_model('prop')`` returns (vae_train.py
    --model-type prop): ``MotifEncoder``, the latent heads, the teacher-forced ``MotifDecoder``.  Same constructor argument
    bag, sub-module names and ``state_dict`` keys.

    ``forward(mols, graphs, tensors, orders, homos, lumos, beta, perturb_z=True, schedule=None) -> (loss, metrics)``:
    loss = (topo + cls + icls + assm) / B + beta * KL; metrics under the reference's keys ('KL:' with its colon).
    """

    HIER = False

    def __init__(self, args):
        super().__init__()
        from .encoder import MotifEncoder
        from .motif_decoder import MotifDecoder
        self._build(args, MotifEncoder, MotifDecoder)


class PropOptVAE(_PropOptVAE):
    """reference ggpm/property_vae.py:257-397 -- the tree-only model ``OPVNet.get_model('prop-opt')`` returns
    (vae_fine_tune_indv_opt.py): PropertyVAE's encoder, rsample and decoder plus the HOMO / LUMO heads and optionally
    ``LossWeigh``, as HierPropOptVAE, with the reference's two differences:
      * the embeddings are ALWAYS tied (the reference's first ``tie_embedding`` call is unconditional);
      * ``beta * KL`` IS added to the reconstruction loss (before ``loss_scaling``), so R_var receives a gradient even
        with ``perturb_z=False``.
    ``forward(...) -> (total_loss, metrics, clipped)`` with HierPropOptVAE's keys, ``clip_negative_loss`` and conventions.
    """

    HIER = False
    KL_IN_LOSS = True

    def __init__(self, args):
        super().__init__()
        from .encoder import MotifEncoder
        from .motif_decoder import MotifDecoder
        self._build(args, MotifEncoder, MotifDecoder, tie_always=True)

    def optimize_recs(self, batch, args=None):
        raise NotImplementedError("PropOptVAE.optimize_recs: the reference's version calls PropertyOptimizer.optimize, "
                                  "which ggpm/property_optimizer.py does not define")
