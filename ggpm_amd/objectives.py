"""What computes or trains on the bound of the four VAEs: ``log_likelihood``, ``bound_loss`` and its ``VARIANTS``, the two
latent accumulators and their result types.  The model is reached through its attributes only (``decoder``, ``R_mean``,
``R_var``, ``_encode``, ``_decode_schedule``, ``HIER``)."""
from collections import namedtuple

import torch

from . import functional as F_
from .decoder_heads import check_no_dropout
from .latent_heads import Plain, _LatentTerms, _encode_heads
from .nnutils import make_cuda
from .prior import check_prior


MolLikelihood = namedtuple("MolLikelihood", ["parts", "kl", "elbo", "iwae", "z", "stats"])
MolLikelihood.__doc__ = """What ``log_likelihood`` returns: fp32 device tensors (none requires grad, nothing is synchronised)
for K samples, B molecules and latent width L.
  parts [K, B, 4]  per sample and molecule the summed row losses of the topology BCE, the motif-class CE, the attachment-class
                   CE (vocabulary mask as in training) and the attachment CE (label 0); 0 where a molecule has no such row
  kl    [B]        -0.5 * sum_j(1 + lv - mean^2 - exp(lv)), lv = -|R_var(h)|: the reference's rsample before its / B
  elbo  [B]        -mean_k(sum of parts[k, i, :]) - kl[i]
  iwae  [B]        logsumexp_k(-nll[k, i] + log p(z_k) - log q(z_k | x_i)) - log K; the single-sample ELBO estimate for K = 1
  z     [K, B, L]  the latents used
  stats            {'encoder_calls', 'atom_level_calls', 'decoder_passes'}: python ints, what the call issued"""


MolObjective = namedtuple("MolObjective", ["parts", "kl", "elbo", "iwae", "z", "weights", "stats"])
MolObjective.__doc__ = """The second value of ``bound_loss``: detached fp32 device tensors, the fields of :class:`MolLikelihood` (bit for
bit what ``log_likelihood`` returns for the same draws) plus ``weights [B]``, the molecule weights used (ones for None)."""


class _ExtendedObjective(MolObjective):
    """:class:`MolObjective`'s seven fields and, as attributes, the keyword-only arguments ``_EXTRAS`` names."""

    _EXTRAS = ()

    def __new__(cls, *fields, **extras):
        if set(extras) != set(cls._EXTRAS):
            raise TypeError("%s takes the keyword arguments %s" % (cls.__name__, ", ".join(cls._EXTRAS)))
        self = super().__new__(cls, *fields)
        self.__dict__.update(extras)
        return self


class FreeBitsObjective(_ExtendedObjective):
    """The second value of ``bound_loss(free_bits=...)``: :class:`MolObjective`'s seven fields (so unpacking it is unchanged)
    and two attributes, ``kl_dims`` (fp32 [L] on the device: klbar_j, the weighted batch mean of every latent column's KL)
    and ``free_bits`` (the float used)."""

    _EXTRAS = ("kl_dims", "free_bits")


class EstimatorObjective(_ExtendedObjective):
    """The second value of ``bound_loss(objective="iwae", estimator="stl" | "dreg")``: :class:`MolObjective`'s seven fields
    (bit-equal to the ``estimator="reparam"`` call's) and three attributes, ``estimator`` (the name used), ``sample_weights``
    (fp32 [K, B] on the device: the normalised importance weights of every molecule's K samples) and ``ess`` (fp32 [B]: the
    effective sample size 1 / sum_k sample_weights^2, between 1 and K); the two tensors are detached."""

    _EXTRAS = ("estimator", "sample_weights", "ess")


class DecompositionObjective(_ExtendedObjective):
    """The second value of ``bound_loss(objective="tcvae")``: :class:`MolObjective`'s seven fields (bit-equal to the
    ``objective="elbo"`` call's on the same draws) and the attributes ``mi``, ``tc``, ``dwkl`` (fp32 [K, B] on the device,
    detached: the index-code mutual information, the total correlation and the dimension-wise KL of every draw), ``alpha``,
    ``beta``, ``gamma`` (the floats that weighed them) and ``dataset_size`` (the int used)."""

    _EXTRAS = ("mi", "tc", "dwkl", "alpha", "beta", "gamma", "dataset_size")


class PriorObjective(_ExtendedObjective):
    """The second value of ``bound_loss(prior=...)``: :class:`MolObjective`'s seven fields -- ``kl``, ``elbo`` and ``iwae`` under
    the prior used -- and two attributes, ``log_prior_ratio`` (fp32 [K, B] on the device, detached: log p(z_k) - log N(z_k; 0, I)
    of every draw) and ``kl_standard`` (fp32 [B]: the analytic KL to the standard normal, ``kl`` of the call without a
    prior)."""

    _EXTRAS = ("log_prior_ratio", "kl_standard")


class PriorEstimatorObjective(EstimatorObjective):
    """:class:`EstimatorObjective` of a call with ``prior=``: its attributes and :class:`PriorObjective`'s two."""

    _EXTRAS = EstimatorObjective._EXTRAS + PriorObjective._EXTRAS


class PriorLikelihood(MolLikelihood):
    """What ``log_likelihood(prior=...)`` returns: :class:`MolLikelihood`'s six fields -- ``kl``, ``elbo`` and ``iwae`` under
    the prior used -- and :class:`PriorObjective`'s two attributes."""

    def __new__(cls, *fields, log_prior_ratio, kl_standard):
        self = super().__new__(cls, *fields)
        self.log_prior_ratio, self.kl_standard = log_prior_ratio, kl_standard
        return self


def _prior_terms(prior, z, kl, logpq, stats):
    """What a prior changes in the latent terms (*A learned prior*): ratio [K, B] = log p(z) - log N(z; 0, I) from
    ONE call on all K draws -> (ratio, logpq + ratio, kl - mean_k ratio: the analytic standard-normal KL corrected by a Monte
    Carlo estimate of E_q[log p - log N]; detached).  ``stats`` gains 'prior_launches', which the backward adds to."""
    stats["prior_launches"] = 0

    def count(n):
        stats["prior_launches"] += n

    ratio = prior.log_ratio(z, count=count)
    with torch.no_grad():
        kl_eff = kl.detach() - ratio.detach().mean(dim=0)
    return ratio, logpq + ratio, kl_eff


ESTIMATORS = ("reparam", "stl", "dreg")


class _BoundObjective(torch.autograd.Function):
    """(parts [K, B, 4], logpq [K, B], kl [B]) -> the weighted K-sample ELBO / IWAE loss (ggpm_bound_objective, which also
    leaves the loss's partial derivatives); the backward hands them on, times the upstream gradient.  It is the first node
    of the pass, so it also arranges that the pass adds into gradients that are already there ONCE (_add_pass_once)."""

    @staticmethod
    def forward(ctx, parts, logpq, kl, w, objective, beta, params):
        loss, c_nll, c_logpq, c_kl = F_.bound_objective(parts, logpq, kl, w, objective, beta)
        ctx.coef = (c_nll, c_logpq, c_kl)
        ctx.params = params
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        if ctx.coef is None:
            raise F_.second_backward("bound objective")
        (c_nll, c_logpq, c_kl), ctx.coef = ctx.coef, None
        _add_pass_once(ctx.params)
        g = dloss.reshape(()).to(torch.float32)
        return (c_nll * g).unsqueeze(-1).expand(-1, -1, 4), c_logpq * g, c_kl * g, None, None, None, None


_SET_ASIDE = []         # (parameter, the gradient it held) of the pass in flight


def _add_pass_once(params) -> None:
    """Called from the first node of a backward pass.  A parameter used in several places (tied embeddings; the encoder's
    gradient through autograd, the decoder's through the deferred queue) receives one addition into ``.grad`` per use, so a
    gradient that is already there would be rounded once per use.  Here the gradients that are there are set aside, the pass
    forms its own total exactly as a pass on fresh gradients does, and the last callback of the pass -- behind the deferred
    flush, the atom level's tail and the stream joins -- adds that total to what was there, once: accumulation costs one
    fp32 rounding per element, and ``.grad`` stays the tensor it was.  Not where gradients are formed inside a flat buffer
    (parallel.FlatGradSync, the encoder's gradient sink): setting ``.grad`` aside would let the pass overwrite it there, so
    those keep the one-addition-per-use form."""
    from . import parallel
    main = torch.cuda.current_stream()

    def add_once():
        held, _SET_ASIDE[:] = list(_SET_ASIDE), []
        base, new = [], []
        for p, b in held:
            if p.grad is not None:
                base.append(b)
                new.append(p.grad)
            p.grad = b
        if base:
            with torch.cuda.stream(main):
                torch._foreach_add_(base, new)

    if _SET_ASIDE:          # a pass that raised never ran its callbacks: what it set aside goes back first
        add_once()
    held = [(p, p.grad) for p in params if p.grad is not None]
    if not held or any(id(p) in parallel._GRAD_SLOTS for p, _ in held):
        return
    for p, _ in held:
        p.grad = None
    _SET_ASIDE.extend(held)
    engine = torch.autograd.Variable._execution_engine

    # queued from inside a callback: behind every callback the nodes of this pass queue
    engine.queue_callback(lambda: engine.queue_callback(add_once))


def _no_dropout(model, what):
    check_no_dropout(model, "%s.%s runs without dropout: call model.eval() first" % (type(model).__name__, what),
                     each_dropout=True)


def _n_samples(name, what, n_samples) -> int:
    """``n_samples`` of ``what`` (the method's name in the message) as an int in 1 .. LIKELIHOOD_MAX_K"""
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= int(n_samples) <= F_.LIKELIHOOD_MAX_K:
        raise ValueError("%s.%s: n_samples %r (1 .. %d)" % (name, what, n_samples, F_.LIKELIHOOD_MAX_K))
    return int(n_samples)


def _likelihood_args(model, what, batch, n_samples, sample_ids, eps, max_cls_size, schedule):
    """The argument checks ``log_likelihood`` and ``bound_loss`` share (``what``: the method's name in the messages) ->
    (class name, decoder, device, K, B, L, schedule, pinned max_cls_size)"""
    from .decoder import _pinned_cls_size
    name, dec = type(model).__name__, model.decoder
    _no_dropout(model, what)
    graphs, tensors, orders = batch[1], batch[2], batch[3]
    B, L = len(orders), model.R_mean.weight.shape[0]
    dev = model.R_mean.weight.device
    K = _n_samples(name, what, n_samples)
    if eps is not None:
        if not isinstance(eps, torch.Tensor) or eps.dtype != torch.float32 or eps.device != dev:
            raise ValueError("%s.%s: eps must be a float32 tensor on %s" % (name, what, dev))
        if tuple(eps.shape) != (K, B, L):
            raise ValueError("%s.%s: eps of shape %s for n_samples %d, %d molecules and latent width %d"
                             % (name, what, tuple(eps.shape), K, B, L))
    if sample_ids is not None and len(sample_ids) != B:
        raise ValueError("%s.%s: %d sample_ids for %d molecules" % (name, what, len(sample_ids), B))
    schedule = model._decode_schedule(graphs, tensors, orders, schedule)
    if schedule is None:
        raise ValueError("%s.%s: the batch carries no graphs (batch[1]) and no schedule= was given: nothing to "
                         "derive the decoder's bookkeeping from" % (name, what))
    return name, dec, dev, K, B, L, schedule, _pinned_cls_size(schedule, max_cls_size)


def _likelihood_atom_level(model, what, tensors, schedule, record_grad):
    """What ``log_likelihood`` and ``bound_loss`` run once for all K draws before their encoder pass, under the caller's grad
    mode: the hierarchical decoder's ``atom_level`` -> (tensors on the device, atom, stats with the encoder pass counted)"""
    tensors = make_cuda(tensors)
    atom = None
    if model.HIER:
        atom = model.decoder.atom_level(schedule, tensors, record_grad=record_grad)
        if atom is None:
            raise NotImplementedError("%s.%s: this batch runs the decoder's step loop (no tree message at all, "
                                      "no AtomPlan, or a batched form switched off in ggpm_amd._dev), which has no "
                                      "per-molecule form" % (type(model).__name__, what))
    return tensors, atom, dict(encoder_calls=1, atom_level_calls=int(atom is not None), decoder_passes=0)


def log_likelihood(model, batch, n_samples=1, seed=None, sample_ids=None, eps=None, max_cls_size=None, schedule=None,
                   prior=None):
    """``log_likelihood`` of the four VAEs (*Per-molecule ELBO and the importance-weighted bound*).

    The encoder, ``R_mean`` / ``R_var`` and -- for the hierarchical decoder -- the atom level run once: under teacher
    forcing none of them depends on the latent draw.  Per sample only ``z_k``, ``W_root``, the tree-side levels and the
    heads run.  ``eps[k, i, :]`` comes from the seeded stream of csrc/sample.hip at site LATENT, keyed by ``seed`` (an int,
    64 bits used; None takes them from torch's default CPU generator), ``sample_ids[i]`` (default ``arange``) and the counter
    ``k * L + column``: a molecule's draws do not depend on its batch, and the first K draws of a larger call are the
    K-sample call's.  ``eps=`` (a fp32 [K, B, L] tensor on the model's device, ``n_samples`` = K) replaces the stream; all
    zeros with K = 1 is the ``perturb_z=False`` latent.  ``max_cls_size``: see ``molecule_losses`` -- None is the training
    convention (the parts then add up to the training loss x B), an int makes numbers comparable across batches.
    ``prior`` (None: the standard normal, or a :class:`~ggpm_amd.prior.MixturePrior` of the latent's width on the model's
    device; DESIGN.md, *A learned prior*): ``kl``, ``elbo`` and ``iwae`` are then under that prior, and the result is a
    :class:`PriorLikelihood`, which adds ``log_prior_ratio`` [K, B] and ``kl_standard`` [B]; one more launch."""
    from .greedy_decode import split_seed
    name, dec, dev, K, B, L, schedule, C = _likelihood_args(model, "log_likelihood", batch, n_samples, sample_ids, eps,
                                                            max_cls_size, schedule)
    prior = check_prior("%s.log_likelihood" % name, prior, L, dev)
    mols, graphs, tensors, orders = batch[0], batch[1], batch[2], batch[3]
    with torch.no_grad():
        tensors, atom, stats = _likelihood_atom_level(model, "log_likelihood", tensors, schedule, record_grad=False)
        _, mean, pre_var = _encode_heads(model, tensors)
        if eps is None:
            lo, hi = split_seed(seed)
            eps = F_.sample_latent_normal(K, B, L, lo, hi, ids=sample_ids, device=dev)
        z, kl, logpq = F_.latent_terms(mean, pre_var, eps)
        parts = torch.empty(K, B, 4, dtype=torch.float32, device=dev)
        for k in range(K):
            zk = z[k]
            dec.molecule_losses(mols, (zk, zk, zk), graphs, tensors, orders, schedule=schedule, max_cls_size=C, atom=atom,
                                out=parts[k])
            stats["decoder_passes"] += 1
        if prior is None:
            elbo, iwae = F_.iwae_finish(parts, logpq, kl)
            return MolLikelihood(parts, kl, elbo, iwae, z, stats)
        ratio, logpq_eff, kl_eff = _prior_terms(prior, z, kl, logpq, stats)
        elbo, iwae = F_.iwae_finish(parts, logpq_eff, kl_eff)
    return PriorLikelihood(parts, kl_eff, elbo, iwae, z, stats, log_prior_ratio=ratio, kl_standard=kl)


class _Bound(Plain):
    """The plain variant of ``bound_loss`` -- the K-sample ELBO or the importance-weighted bound, reparameterised -- and the
    base of the others.  A variant checks the call's arguments (``name``: the model's class in the messages), is the
    ``variant`` of the latent-terms node (``extras`` / ``backward``, see latent_heads.Plain; ``w``, the molecule weights, is
    set before), forms the loss from the K decoder passes and wraps the seven common fields in its result type; ``extras`` in
    the last two are the further outputs of its node."""

    def __init__(self, name, B, L, objective, beta, alpha, gamma, dataset_size, free_bits, prior=None):
        if alpha is not None or gamma is not None or dataset_size is not None:
            raise ValueError("%s.bound_loss: alpha, gamma and dataset_size weigh the split KL of objective \"tcvae\"; objective %r "
                             "has none" % (name, objective))
        self.objective, self.beta, self.free_bits, self.w = objective, float(beta), free_bits, None
        if objective == "iwae" and self.beta != 1.0:
            raise ValueError("%s.bound_loss: the importance-weighted bound has no beta (got %r): pass beta=1.0" % (name, self.beta))
        if free_bits is not None:
            if objective != "elbo":
                raise ValueError("%s.bound_loss: free_bits holds the KL of the ELBO; objective %r has none to hold" % (name, objective))
            if prior is not None:
                raise ValueError("%s.bound_loss: free_bits holds the per-column KL to the standard normal, which a prior= "
                                 "replaces; a mixture's KL has no per-column form" % name)
            self.free_bits = float(free_bits)
            if not (0.0 <= self.free_bits < float("inf")):
                raise ValueError("%s.bound_loss: free_bits %r (None, or a finite value >= 0)" % (name, self.free_bits))
            if L > F_.FREE_BITS_MAX_L:
                raise ValueError("%s.bound_loss: free_bits for %d latent columns (at most %d)" % (name, L, F_.FREE_BITS_MAX_L))

    def loss(self, parts, logpq, kl, extras, params):
        return _BoundObjective.apply(parts, logpq, kl, self.w, self.objective, self.beta, params)

    def info(self, fields, extras):
        return MolObjective(*fields)


class _FreeBits(_Bound):
    """The ELBO with the free-bits KL beside it: the node also returns ``term = sum_j max(free_bits, klbar_j)`` and
    ``kl_dims`` (ggpm_free_bits_kl; ``w`` weighs the molecules in klbar).  On the way back ggpm_free_bits_kl_backward's
    dmean / dpre_var are added to ggpm_latent_terms_backward's, so the heads and their deferred weight gradients run once.
    ``term`` reaches parameters only through this node, which also waits for z, kl and logpq: _BoundObjective stays the first
    node of the pass."""

    def extras(self, ctx, z, mean, pv):
        kl_dims, term = F_.free_bits_kl(mean, pv, self.w, self.free_bits)
        ctx.mark_non_differentiable(kl_dims)
        return (term.reshape(()), kl_dims), (kl_dims,)

    def backward(self, dz, dkl, dlogpq, dextras, mean, pv, eps, saved):
        dmean, dpv = F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)
        dterm, (kl_dims,) = dextras[0], saved
        if dterm is not None:
            fm, fp = F_.free_bits_kl_backward(mean, pv, self.w, self.free_bits, dterm.reshape(1).to(torch.float32), kl_dims)
            dmean.add_(fm)
            dpv.add_(fp)
        return dmean, dpv

    def loss(self, parts, logpq, kl, extras, params):
        # the reconstruction part is the ELBO without its KL; the held KL joins it as one term
        return _BoundObjective.apply(parts, logpq, kl, self.w, "elbo", 0.0, params) + self.beta * extras[0]

    def info(self, fields, extras):
        return FreeBitsObjective(*fields, kl_dims=extras[1].detach(), free_bits=self.free_bits)


class _TCVAE(_Bound):
    """The beta-TCVAE loss, with the KL split across the batch beside the latent terms: the node also returns ``comps``
    [K, B, 3] -- the index-code mutual information, the total correlation and the dimension-wise KL of every draw
    (ggpm_latent_decomp on the z, mean and pre_var of this very node; ``dataset_size`` is N of log(N B)).  On the way back
    ggpm_latent_decomp_backward turns the gradient that reached ``comps`` into dz, dmean and dpre_var with the three held
    independent; its dz joins the decoder's before ggpm_latent_terms_backward -- the existing rsample chain -- and its
    dmean / dpre_var are added behind it, so the heads and their deferred weight gradients run once."""

    def __init__(self, name, B, L, objective, beta, alpha, gamma, dataset_size, free_bits, prior=None):
        if free_bits is not None:
            raise ValueError("%s.bound_loss: free_bits holds the KL of the ELBO; objective \"tcvae\" splits it instead" % name)
        if prior is not None:
            raise ValueError("%s.bound_loss: objective \"tcvae\" splits the KL to the standard normal (its dimension-wise part "
                             "is against N(0, 1) column by column), which a prior= replaces" % name)
        if dataset_size is None:
            raise ValueError("%s.bound_loss: objective \"tcvae\" needs dataset_size, the number of molecules of the data set"
                             % name)
        F_.latent_decomp_log_nb("%s.bound_loss" % name, dataset_size, B)
        alpha, gamma = 1.0 if alpha is None else float(alpha), 1.0 if gamma is None else float(gamma)
        for what, v in (("alpha", alpha), ("beta", float(beta)), ("gamma", gamma)):
            if not (abs(v) < float("inf")):
                raise ValueError("%s.bound_loss: %s %r (a finite weight)" % (name, what, v))
        if B > F_.LATENT_DECOMP_MAX_B or L > F_.FREE_BITS_MAX_L:
            raise ValueError("%s.bound_loss: objective \"tcvae\" for %d molecules and %d latent columns (at most %d and %d)"
                             % (name, B, L, F_.LATENT_DECOMP_MAX_B, F_.FREE_BITS_MAX_L))
        self.alpha, self.beta, self.gamma, self.dataset_size, self.w = alpha, float(beta), gamma, dataset_size, None

    def extras(self, ctx, z, mean, pv):
        comps, _, lse_joint, lse_dim = F_.latent_decomposition(z, mean, pv, self.dataset_size)
        return (comps,), (z, lse_joint, lse_dim)

    def backward(self, dz, dkl, dlogpq, dextras, mean, pv, eps, saved):
        dcomps, (z, lse_joint, lse_dim) = dextras[0], saved
        if dcomps is not None:
            cz, cm, cp = F_.latent_decomposition_backward(z, mean, pv, lse_joint, lse_dim, dcomps.to(torch.float32))
            dz = cz if dz is None else cz.add_(dz)
        dmean, dpv = F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)
        if dcomps is not None:
            dmean.add_(cm)
            dpv.add_(cp)
        return dmean, dpv

    def loss(self, parts, logpq, kl, extras, params):
        # the reconstruction part is the ELBO without its KL; the three components join it as one weighted sum (formed in
        # fp64: tc and dwkl carry +- L log(N B), which cancels between them)
        (K, B, _), dev, w = parts.shape, parts.device, self.w
        cw = (torch.ones(B, dtype=torch.float64, device=dev) if w is None else w.double()) / float(B * K)
        cw = cw[None, :, None] * torch.tensor([self.alpha, self.beta, self.gamma], dtype=torch.float64, device=dev)
        return _BoundObjective.apply(parts, logpq, kl, w, "elbo", 0.0, params) + (extras[0].double() * cw).sum().to(torch.float32)

    def info(self, fields, extras):
        c = extras[0].detach()
        return DecompositionObjective(*fields, mi=c[..., 0], tc=c[..., 1], dwkl=c[..., 2], alpha=self.alpha, beta=self.beta,
                                      gamma=self.gamma, dataset_size=self.dataset_size)


class _Path(_Bound):
    """The path-derivative estimators of the importance-weighted bound: the same forward, and on the way back
    ggpm_latent_terms_backward_path -- the parameters of log q held fixed, for DReG every sample weighted by ``s`` -- then
    _KLHead's tail.  The gradient that arrives for kl is c_kl g = 0 for the importance-weighted bound and takes no part.
    ``s`` [K, B], the normalised importance weights, and ``ess`` [B], the effective sample sizes (ggpm_iwae_weights), exist
    only once the K decoder passes have run: ``loss`` fills them in and the node's backward, which runs once, reads ``s``."""

    ESTIMATOR, DREG = "stl", False

    def __init__(self, name, B, L, objective, beta, alpha, gamma, dataset_size, free_bits, prior=None):
        if objective != "iwae":
            raise ValueError("%s.bound_loss: estimator %r changes the gradient of the importance-weighted bound; objective %r "
                             "has an analytic KL and no score term to remove (free_bits included)"
                             % (name, self.ESTIMATOR, objective))
        super().__init__(name, B, L, objective, beta, alpha, gamma, dataset_size, free_bits, prior)
        self.s, self.ess, self.spent = None, None, False

    def backward(self, dz, dkl, dlogpq, dextras, mean, pv, eps, saved):
        if self.spent:
            raise F_.second_backward("path latent terms")
        self.spent = True
        return F_.latent_terms_backward_path(dz, mean, pv, eps, dlogpq, self.s if self.DREG else None)

    def loss(self, parts, logpq, kl, extras, params):
        with torch.no_grad():
            self.s, self.ess = F_.iwae_weights(parts.detach(), logpq.detach())
        return super().loss(parts, logpq, kl, extras, params)

    def info(self, fields, extras):
        return EstimatorObjective(*fields, estimator=self.ESTIMATOR, sample_weights=self.s, ess=self.ess)


class _DReG(_Path):
    ESTIMATOR, DREG = "dreg", True


# what differs between the modes of ``bound_loss``, in one entry each; a call of ``bound_loss`` picks its entry once
VARIANTS = {"plain": _Bound, "free_bits": _FreeBits, "tcvae": _TCVAE, "stl": _Path, "dreg": _DReG}


def bound_loss(model, batch, n_samples=1, objective="elbo", beta=1.0, mol_weights=None, seed=None, sample_ids=None, eps=None,
               max_cls_size=None, schedule=None, estimator="reparam", prior=None, alpha=None, gamma=None, dataset_size=None,
               free_bits=None):
    """``bound_loss`` of the four VAEs (*Training on the bound*) -> (loss, :class:`MolObjective`).

    With ``nll``, ``kl``, ``logpq`` and ``iwae`` as ``log_likelihood`` forms them, w the molecule weights and K = n_samples:
      objective="elbo":  loss = (1/B) sum_i w_i ((1/K) sum_k nll[k, i] + beta kl[i])
      objective="iwae":  loss = -(1/B) sum_i w_i iwae[i]                                    (beta must be 1.0)
    ``loss`` is a 0-dim tensor autograd differentiates: the reparameterised gradient through the decoder, through
    z_k = mean + exp(lv / 2) eps_k, through the lv and z terms of logpq and through kl, to every encoder, latent-head and
    decoder parameter (the property heads and LossWeigh of the -opt models take no part).  ``mol_weights``: None or B
    floats (a host sequence or a float32 tensor on the model's device), a constant.  Every other argument is
    ``log_likelihood``'s.  One encoder pass and one atom-level pass serve the K decoder passes, forward and backward.

    ``free_bits`` (None, or a finite float >= 0 with ``objective="elbo"``; DESIGN.md, *Per-dimension KL*): the KL is held
    per latent column instead of per molecule,
      loss = (1/B) sum_i w_i (1/K) sum_k nll[k, i] + beta sum_j max(free_bits, klbar_j),  klbar_j = (1/B) sum_i w_i kl_dim[i, j]
    so a column whose batch-mean KL is at or below ``free_bits`` nats is no longer pushed down (its KL gradient is exactly
    zero).  ``free_bits=0.0`` is the ELBO above summed in another order.  The second value is then a
    :class:`FreeBitsObjective`, which adds ``kl_dims`` ([L], klbar) and ``free_bits`` to the same seven fields.

    ``objective="tcvae"`` (*Splitting the KL*): the beta-TCVAE loss, which weighs the three parts of the KL
    separately,
      loss = (1/B) sum_i w_i (1/K) sum_k (nll[k, i] + alpha mi[k, i] + beta tc[k, i] + gamma dwkl[k, i])
    with mi the index-code mutual information, tc the total correlation and dwkl the dimension-wise KL of draw (k, i),
    estimated by minibatch-weighted sampling from the B posteriors of the batch and ``dataset_size`` (required: an int >= B,
    the number of molecules of the data set).  ``alpha`` and ``gamma`` default to 1.0 (None); all three weights must be
    finite.  mi + tc + dwkl = log q(z_k | x_i) - log p(z_k) exactly, so alpha = beta = gamma = 1 is the single-sample
    estimate of the ELBO.  ``mol_weights`` weigh the outer sum over molecules only: the estimate of q(z) uses every molecule
    of the batch unweighted.  ``estimator`` must be "reparam" and ``free_bits`` None.  The second value is a
    :class:`DecompositionObjective`, which adds ``mi``, ``tc``, ``dwkl`` ([K, B]), ``alpha``, ``beta``, ``gamma`` and
    ``dataset_size`` to the same seven fields.

    ``estimator`` (*STL and DReG*): how the gradient of the importance-weighted bound reaches the encoder and
    ``R_mean`` / ``R_var``.  ``"reparam"``, the default, is the gradient described above.  ``"stl"`` ("sticking the landing")
    holds the posterior's parameters fixed inside log q(z_k | x), which removes the zero-mean score term whose variance
    does not shrink with K; it is biased for K > 1.  ``"dreg"`` (doubly reparameterised) weighs every sample of that path
    gradient by its normalised importance weight once more and is unbiased.  Both need ``objective="iwae"`` (the analytic
    KL of the ELBO has no score term to remove, so ``free_bits`` is excluded too); loss, ``info``'s seven fields and the
    decoder's gradients are those of ``"reparam"``, and the second value is an :class:`EstimatorObjective`, which adds
    ``estimator``, ``sample_weights`` ([K, B]) and ``ess`` ([B]).

    ``prior`` (*A learned prior*): None is the standard normal, the call as it is without the argument.  A
    :class:`~ggpm_amd.prior.MixturePrior` of the latent's width on the model's device replaces it: with
    ratio[k, i] = log p(z_k) - log N(z_k; 0, I) from one call on all K draws,
      logpq_eff = logpq + ratio          kl_eff[i] = kl[i] - (1/K) sum_k ratio[k, i]
    stand where logpq and kl stand above, and the gradient also reaches the prior's three parameters and, through z, the
    encoder (under "stl" / "dreg" as part of the path term, not of the log q held fixed).  ``free_bits`` and
    ``objective="tcvae"`` are defined against the standard normal and raise with a prior.  The second value is then a
    :class:`PriorObjective` (:class:`PriorEstimatorObjective` under "stl" / "dreg"), which adds ``log_prior_ratio`` ([K, B])
    and ``kl_standard`` ([B]); ``stats`` gains 'prior_launches', 1 after the forward and at most 3 after the backward."""
    from .greedy_decode import split_seed
    name, dec, dev, K, B, L, schedule, C = _likelihood_args(model, "bound_loss", batch, n_samples, sample_ids, eps,
                                                            max_cls_size, schedule)
    prior = check_prior("%s.bound_loss" % name, prior, L, dev)
    if objective not in F_.BOUND_OBJECTIVES and objective != "tcvae":
        raise ValueError("%s.bound_loss: objective %r (one of %s)" % (name, objective, sorted(F_.BOUND_OBJECTIVES) + ["tcvae"]))
    if estimator not in ESTIMATORS:
        raise ValueError("%s.bound_loss: estimator %r (one of %s)" % (name, estimator, ", ".join(ESTIMATORS)))
    reparam = "tcvae" if objective == "tcvae" else "plain" if free_bits is None else "free_bits"
    variant = VARIANTS[estimator if estimator != "reparam" else reparam](name, B, L, objective, beta, alpha, gamma, dataset_size,
                                                                       free_bits, prior)
    w = None
    if mol_weights is not None:
        if isinstance(mol_weights, torch.Tensor):
            if mol_weights.dtype != torch.float32 or mol_weights.device != dev:
                raise ValueError("%s.bound_loss: mol_weights must be a float32 tensor on %s (or a host sequence)" % (name, dev))
            w = mol_weights.detach()
        else:
            w = torch.as_tensor([float(v) for v in mol_weights], dtype=torch.float32).to(dev)
        if tuple(w.shape) != (B,):
            raise ValueError("%s.bound_loss: %d mol_weights for %d molecules" % (name, w.numel(), B))
    variant.w = w
    mols, graphs, tensors, orders = batch[0], batch[1], batch[2], batch[3]
    with torch.enable_grad():
        tensors, atom, stats = _likelihood_atom_level(model, "bound_loss", tensors, schedule, record_grad=True)
        root_vecs = model._encode(tensors)
        if eps is None:
            lo, hi = split_seed(seed)
            eps = F_.sample_latent_normal(K, B, L, lo, hi, ids=sample_ids, device=dev)
        Rm, Rv = model.R_mean, model.R_var
        z, kl, logpq, *extras = _LatentTerms.apply(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias, eps.detach(), variant)
        parts = []
        for k in range(K):
            zk = z[k]
            parts.append(dec.molecule_losses(mols, (zk, zk, zk), graphs, tensors, orders, schedule=schedule, max_cls_size=C,
                                             atom=atom))
            stats["decoder_passes"] += 1
        parts = torch.stack(parts, dim=0)
        if prior is None:
            loss = variant.loss(parts, logpq, kl, extras, tuple(model.parameters()))
            kl_eff = kl.detach()
        else:
            ratio, logpq, kl_eff = _prior_terms(prior, z, kl, logpq, stats)
            # the ELBO's KL is beta kl_eff: the objective's beta kl and one weighted sum of ratio (formed before the objective,
            # which stays the first node of the pass); the importance-weighted bound reads ratio inside logpq_eff
            term = None
            if objective == "elbo":
                cw = (torch.ones(B, dtype=torch.float64, device=dev) if w is None else w.double()) * (-variant.beta / float(B * K))
                term = (ratio.double() * cw[None, :]).sum().to(torch.float32)
            loss = variant.loss(parts, logpq, kl, extras, tuple(model.parameters()))
            loss = loss if term is None else loss + term
    with torch.no_grad():
        elbo, iwae = F_.iwae_finish(parts.detach(), logpq.detach(), kl_eff)
    ones = w if w is not None else torch.ones(B, dtype=torch.float32, device=dev)
    info = variant.info((parts.detach(), kl_eff, elbo, iwae, z.detach(), ones, stats), extras)
    if prior is not None:
        cls = PriorEstimatorObjective if isinstance(info, EstimatorObjective) else PriorObjective
        info = cls(*info, log_prior_ratio=ratio.detach(), kl_standard=kl.detach(), **getattr(info, "__dict__", {}))
    return loss, info


def _update_heads(model, what, batch):
    """How both accumulators begin an update: no active dropout, then (mean, pre_var) of the molecules of ``batch``"""
    _no_dropout(model, what)
    return _encode_heads(model, make_cuda(batch[2]))[1:]


LatentStats = namedtuple("LatentStats", ["kl_dims", "mu_mean", "mu_var", "sigma2_mean", "agg_var", "n_active", "n_molecules"])
LatentStats.__doc__ = """What ``latent_stats`` and ``LatentAccumulator.result`` return, over the N molecules seen and per latent column j
(fp32 [L] device tensors; nothing requires grad, nothing is synchronised), with lv = -|R_var(h)| and mean = R_mean(h):
  kl_dims      mean over molecules of -0.5 (1 + lv - mean^2 - exp(lv)); summed over j it is the mean of ``log_likelihood``'s kl
  mu_mean      mean over molecules of mean
  mu_var       population variance over molecules of mean: Var_x E_q[z_j], the quantity behind "active units"
  sigma2_mean  mean over molecules of exp(lv), the posterior variance
  agg_var      mu_var + sigma2_mean, the variance of the aggregate posterior (1 where it matches the prior)
  n_active     0-dim int32 device tensor: the columns with mu_var > au_threshold
  n_molecules  python int: N, counted on the host"""


class LatentAccumulator:
    """Per-dimension statistics of a model's latent over any number of batches (``model.latent_accumulator()``).  The sums
    stay on the device in fp64 (ggpm_latent_dim_accumulate adds one batch per launch; nothing is synchronised);
    ``result()`` may be called at any time and updates may go on after it."""

    def __init__(self, model, au_threshold=0.01):
        self.model, self.au_threshold = model, float(au_threshold)
        if self.au_threshold != self.au_threshold:
            raise ValueError("%s.latent_accumulator: au_threshold is NaN" % type(model).__name__)
        _no_dropout(model, "latent_stats")
        Rm = model.R_mean.weight
        self.acc = torch.zeros(F_.LATENT_STAT_ROWS, Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.n_molecules = 0

    def update(self, batch):
        """Adds the molecules of ``batch`` (the tuple ``model(*batch)`` takes; only ``batch[2]``, the tensors, is used)."""
        with torch.no_grad():
            mean, pre_var = _update_heads(self.model, "latent_stats", batch)
            F_.latent_dim_accumulate(mean, pre_var, self.acc)
        self.n_molecules += mean.shape[0]
        return self

    def result(self):
        """-> :class:`LatentStats` of what has been added so far (zeros before the first update)"""
        out, n_active = F_.latent_dim_finish(self.acc, self.au_threshold)
        return LatentStats(out[0], out[1], out[2], out[3], out[4], n_active.reshape(()), self.n_molecules)


LatentDecomposition = namedtuple("LatentDecomposition", ["mi", "tc", "dwkl", "dwkl_dims", "kl", "n_molecules"])
LatentDecomposition.__doc__ = """What ``latent_decomposition`` and ``LatentDecompositionAccumulator.result`` return: means over the
draws of the N molecules seen (fp32 device tensors; nothing requires grad, nothing is synchronised).
  mi           0-dim: the index-code mutual information I(x; z), E[log q(z|x) - log q(z)]
  tc           0-dim: the total correlation KL(q(z) || prod_l q(z_l))
  dwkl         0-dim: the dimension-wise KL sum_l KL(q(z_l) || p(z_l))
  dwkl_dims    [L]: the dimension-wise KL column by column (it sums to ``dwkl``)
  kl           0-dim: the mean over molecules of the analytic KL(q(z|x) || p(z)), which mi + tc + dwkl estimates
  n_molecules  python int: N, counted on the host
log q(z) and log q(z_l) are minibatch-weighted estimates from the molecules of the draw's own batch and ``dataset_size``;
they are biased for small batches (DESIGN.md, *Splitting the KL*)."""


class LatentDecompositionAccumulator:
    """The split of the KL over any number of batches (``model.latent_decomposition_accumulator(dataset_size)``).  Every
    update draws ``n_samples`` latents per molecule from the seeded stream -- molecule n of the pass has sample id n, so no
    two batches share draws -- and adds the batch's sums on the device in fp64 (ggpm_latent_decomp, then
    ggpm_latent_decomp_accumulate and, for the analytic KL, ggpm_latent_dim_accumulate; nothing is synchronised).
    ``result()`` may be called at any time and updates may go on after it."""

    def __init__(self, model, dataset_size, n_samples=1, seed=None):
        from .greedy_decode import split_seed
        name = type(model).__name__
        self.model = model
        _no_dropout(model, "latent_decomposition")
        F_.latent_decomp_log_nb("%s.latent_decomposition" % name, dataset_size, 1)
        self.dataset_size, self.n_samples = dataset_size, _n_samples(name, "latent_decomposition", n_samples)
        self.seed = split_seed(seed)
        Rm = model.R_mean.weight
        self.acc = torch.zeros(F_.LATENT_DECOMP_ROWS + Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.dims = torch.zeros(F_.LATENT_STAT_ROWS, Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.n_molecules = 0

    def update(self, batch):
        """Adds the molecules of ``batch`` (the tuple ``model(*batch)`` takes; only ``batch[2]``, the tensors, is used)."""
        with torch.no_grad():
            mean, pre_var = _update_heads(self.model, "latent_decomposition", batch)
            B, L = mean.shape
            F_.latent_decomp_log_nb("%s.latent_decomposition" % type(self.model).__name__, self.dataset_size, B)
            ids = torch.arange(self.n_molecules, self.n_molecules + B, dtype=torch.int64)
            eps = F_.sample_latent_normal(self.n_samples, B, L, self.seed[0], self.seed[1], ids=ids, device=mean.device)
            z, _, _ = F_.latent_terms(mean, pre_var, eps)
            comps, dwkl_dim, _, _ = F_.latent_decomposition(z, mean, pre_var, self.dataset_size)
            F_.latent_decomp_accumulate(comps, dwkl_dim, self.acc)
            F_.latent_dim_accumulate(mean, pre_var, self.dims)
        self.n_molecules += B
        return self

    def result(self):
        """-> :class:`LatentDecomposition` of what has been added so far (zeros before the first update)"""
        with torch.no_grad():
            n = self.acc[0]
            out = torch.where(n > 0, self.acc[1:] / n.clamp(min=1.0), torch.zeros_like(self.acc[1:])).to(torch.float32)
            kl = F_.latent_dim_finish(self.dims)[0][0].sum()
        return LatentDecomposition(out[0], out[1], out[2], out[3:], kl, self.n_molecules)
