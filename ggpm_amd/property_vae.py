"""Encoder half of the reference's HierPropertyVAE (ggpm/property_vae.py:11-62): encoder + latent heads + KL.

The decoder is outside this build's scope.  ``rsample`` restates
ggpm/property_vae.py:26-33; the two [B,H]x[H,latent] products run through the library GEMM, the
[B,latent] elementwise tail (|.|, exp, KL sum, reparameterisation) is one HIP launch each way (csrc/losses.hip).
"""
from __future__ import annotations

import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import _dev
from . import functional as F_
from .decoder_heads import check_no_dropout
from .encoder import HierMPNEncoder
from .nnutils import make_cuda


class _RsampleTail(torch.autograd.Function):
    """(mean, pv, eps) -> (z, kl): the elementwise part of rsample in one launch each way (csrc/losses.hip)."""

    @staticmethod
    def forward(ctx, mean, pv, eps):
        from . import _lib
        B, L = mean.shape
        mean, pv = mean.contiguous(), pv.contiguous()
        eps = eps.contiguous() if eps is not None else None
        z = torch.empty_like(mean)
        kl = torch.empty(1, dtype=torch.float32, device=mean.device)
        _lib.check(_lib.load().ggpm_rsample_forward(F_._p(mean), F_._p(pv), F_._p(eps), B, L, F_._p(z), F_._p(kl),
                                                    F_._stream()), "rsample_forward")
        ctx.save_for_backward(mean, pv)
        ctx.eps = eps
        return z, kl.reshape(())

    @staticmethod
    def backward(ctx, dz, dkl):
        from . import _lib
        mean, pv = ctx.saved_tensors
        B, L = mean.shape
        dz = dz.contiguous() if dz is not None else None
        dkl = dkl.reshape(1).contiguous() if dkl is not None else None
        dmean, dpv = torch.empty_like(mean), torch.empty_like(pv)
        _lib.check(_lib.load().ggpm_rsample_backward(F_._p(mean), F_._p(pv), F_._p(ctx.eps), F_._p(dz), F_._p(dkl), B, L,
                                                     F_._p(dmean), F_._p(dpv), F_._stream()), "rsample_backward")
        return dmean, dpv, None


def _latent_heads(z_vecs, Wm, bm, Wv, bv):
    """(mean, pre_var) = (R_mean(h), R_var(h)): both [B,H]x[H,latent] products in one grouped launch"""
    B, (L, H) = z_vecs.shape[0], Wm.shape
    mean = torch.empty(B, L, dtype=torch.float32, device=z_vecs.device)
    pv = torch.empty(B, L, dtype=torch.float32, device=z_vecs.device)
    F_.gemm_grouped(0, 1, B, L, H, [
        dict(A=z_vecs, lda=F_._ld(z_vecs), B=Wm, ldb=Wm.stride(0), C=mean, ldc=L, n_pad=L, bias=bm),
        dict(A=z_vecs, lda=F_._ld(z_vecs), B=Wv, ldb=Wv.stride(0), C=pv, ldc=L, n_pad=L, bias=bv)])
    return mean, pv


class _KLHead(torch.autograd.Function):
    """The whole of rsample as ONE autograd node: both [B,H]x[H,latent] products in one grouped launch, the elementwise
    tail in one launch, and on the way back one launch for d(z_vecs) (two K segments), one grouped launch for the two
    weight gradients (second stream, straight into ``.grad`` like the level functions do)."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps):
        from . import _lib
        B, (L, H) = z_vecs.shape[0], Wm.shape
        dev = z_vecs.device
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z = torch.empty_like(mean)
        kl = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().ggpm_rsample_forward(F_._p(mean), F_._p(pv), F_._p(eps), B, L, F_._p(z), F_._p(kl),
                                                    F_._stream()), "rsample_forward")
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv)
        ctx.eps = eps
        ctx.params = (Wm, bm, Wv, bv)           # the Parameter objects themselves (their .grad is assigned)
        return z, kl.reshape(())

    @staticmethod
    def backward(ctx, dz, dkl):
        from . import _lib
        z_vecs, Wm, Wv, mean, pv = ctx.saved_tensors
        B, (L, H) = z_vecs.shape[0], Wm.shape
        dz = dz.contiguous() if dz is not None else None
        dkl = dkl.reshape(1).contiguous() if dkl is not None else None
        dmean, dpv = torch.empty_like(mean), torch.empty_like(pv)
        _lib.check(_lib.load().ggpm_rsample_backward(F_._p(mean), F_._p(pv), F_._p(ctx.eps), F_._p(dz), F_._p(dkl), B, L,
                                                     F_._p(dmean), F_._p(dpv), F_._stream()), "rsample_backward")
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None,)


def _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv):
    """(dmean, dpre_var) -> the gradients of (z_vecs, Wm, bm, Wv, bv): one launch for d(z_vecs) (two K segments), one grouped
    launch for the two weight gradients (second stream, straight into ``.grad``, where they can be published).
    ``ctx.params``: the four Parameter objects."""
    B, (L, H) = z_vecs.shape[0], Wm.shape
    dx = None
    if ctx.needs_input_grad[0]:
        dx = torch.empty_like(z_vecs)
        F_.gemm_ksegments(0, B, H, [dmean, dpv], [L, L], [Wm, Wv], [Wm.stride(0), Wv.stride(0)], [L, L], dx,
                          F_._ld(dx), z_vecs.shape[1])

    def param_grads():
        dWm, dWv = torch.empty_like(Wm), torch.empty_like(Wv)
        F_.gemm_grouped(1, 0, L, H, B, [
            dict(A=dmean, lda=L, B=z_vecs, ldb=F_._ld(z_vecs), C=dWm, ldc=dWm.stride(0), n_pad=H),
            dict(A=dpv, lda=L, B=z_vecs, ldb=F_._ld(z_vecs), C=dWv, ldc=dWv.stride(0), n_pad=H)])
        return dWm, F_.colsum(dmean, B, L), dWv, F_.colsum(dpv, B, L)

    if F_.side_stream_enabled() and F_.can_publish(*ctx.params) and all(ctx.needs_input_grad[1:5]):
        main = torch.cuda.current_stream()
        side = F_._side_stream(z_vecs.device)
        side.wait_stream(main)
        for t in (dmean, dpv, z_vecs):
            t.record_stream(side)
        with torch.cuda.stream(side):
            for q, g in zip(ctx.params, param_grads()):
                F_._accumulate_grad(q, g, main)
        F_._join_later(main, side)
        return dx, None, None, None, None
    dWm, dbm, dWv, dbv = param_grads()
    return dx, dWm, dbm, dWv, dbv


class _LatentTerms(torch.autograd.Function):
    """_KLHead for K draws per molecule: (z_vecs, R_mean, R_var, eps [K, B, L]) -> (z [K, B, L], kl [B], logpq [K, B]) --
    ``_latent_heads`` and ggpm_latent_terms, the launches of ``log_likelihood`` -- and on the way back
    ggpm_latent_terms_backward (the K gradients of z, of logpq and of kl summed in a fixed order), then _KLHead's tail."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z, kl, logpq = F_.latent_terms(mean, pv, eps)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv, eps)
        ctx.params = (Wm, bm, Wv, bv)
        ctx.set_materialize_grads(False)
        return z, kl, logpq

    @staticmethod
    def backward(ctx, dz, dkl, dlogpq):
        z_vecs, Wm, Wv, mean, pv, eps = ctx.saved_tensors
        dmean, dpv = F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None,)


class _FreeBitsLatentTerms(torch.autograd.Function):
    """_LatentTerms with the free-bits KL beside it: also returns ``term = sum_j max(free_bits, klbar_j)`` and ``kl_dims``
    (ggpm_free_bits_kl; ``w`` [B] or None weighs the molecules in klbar).  On the way back ggpm_free_bits_kl_backward's
    dmean / dpre_var are added to ggpm_latent_terms_backward's, so the heads and their deferred weight gradients run once.
    ``term`` reaches parameters only through this node, which also waits for z, kl and logpq: _BoundObjective stays the first
    node of the pass."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps, w, free_bits):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z, kl, logpq = F_.latent_terms(mean, pv, eps)
        kl_dims, term = F_.free_bits_kl(mean, pv, w, free_bits)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv, eps, kl_dims)
        ctx.params = (Wm, bm, Wv, bv)
        ctx.free_bits = (w, free_bits)
        ctx.mark_non_differentiable(kl_dims)
        ctx.set_materialize_grads(False)
        return z, kl, logpq, term.reshape(()), kl_dims

    @staticmethod
    def backward(ctx, dz, dkl, dlogpq, dterm, _):
        z_vecs, Wm, Wv, mean, pv, eps, kl_dims = ctx.saved_tensors
        dmean, dpv = F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)
        if dterm is not None:
            w, free_bits = ctx.free_bits
            fm, fp = F_.free_bits_kl_backward(mean, pv, w, free_bits, dterm.reshape(1).to(torch.float32), kl_dims)
            dmean.add_(fm)
            dpv.add_(fp)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None, None, None)


class _DecompLatentTerms(torch.autograd.Function):
    """_LatentTerms with the KL split across the batch beside it: also returns ``comps`` [K, B, 3] -- the index-code mutual
    information, the total correlation and the dimension-wise KL of every draw (ggpm_latent_decomp on the z, mean and pre_var
    of this very node; ``dataset_size`` is N of log(N B)).  On the way back ggpm_latent_decomp_backward turns the gradient
    that reached ``comps`` into dz, dmean and dpre_var with the three held independent; its dz joins the decoder's before
    ggpm_latent_terms_backward -- the existing rsample chain -- and its dmean / dpre_var are added behind it, so the heads
    and their deferred weight gradients run once."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps, dataset_size):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z, kl, logpq = F_.latent_terms(mean, pv, eps)
        comps, _, lse_joint, lse_dim = F_.latent_decomposition(z, mean, pv, dataset_size)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv, eps, z, lse_joint, lse_dim)
        ctx.params = (Wm, bm, Wv, bv)
        ctx.set_materialize_grads(False)
        return z, kl, logpq, comps

    @staticmethod
    def backward(ctx, dz, dkl, dlogpq, dcomps):
        z_vecs, Wm, Wv, mean, pv, eps, z, lse_joint, lse_dim = ctx.saved_tensors
        if dcomps is not None:
            cz, cm, cp = F_.latent_decomposition_backward(z, mean, pv, lse_joint, lse_dim, dcomps.to(torch.float32))
            dz = cz if dz is None else cz.add_(dz)
        dmean, dpv = F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)
        if dcomps is not None:
            dmean.add_(cm)
            dpv.add_(cp)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None, None)


class _ImportanceWeights:
    """What ``bound_loss`` hands to _PathLatentTerms when it applies it and fills in after the K decoder passes: the normalised
    importance weights ``s`` [K, B] and the effective sample sizes ``ess`` [B] (ggpm_iwae_weights), which exist only once the
    passes have run; ``dreg``: whether the node's backward weighs every sample by ``s`` once more."""

    def __init__(self, dreg):
        self.dreg, self.s, self.ess = bool(dreg), None, None


class _PathLatentTerms(torch.autograd.Function):
    """_LatentTerms for the path-derivative estimators of the importance-weighted bound: the same forward, and on the way back
    ggpm_latent_terms_backward_path -- the parameters of log q held fixed, for DReG every sample weighted by ``weights.s`` --
    then _KLHead's tail.  The gradient that arrives for kl is c_kl g = 0 for the importance-weighted bound and takes no part."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps, weights):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z, kl, logpq = F_.latent_terms(mean, pv, eps)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv, eps)
        ctx.params = (Wm, bm, Wv, bv)
        ctx.weights = weights
        ctx.set_materialize_grads(False)
        return z, kl, logpq

    @staticmethod
    def backward(ctx, dz, dkl, dlogpq):
        if ctx.weights is None:
            raise F_.second_backward("path latent terms")
        weights, ctx.weights = ctx.weights, None
        z_vecs, Wm, Wv, mean, pv, eps = ctx.saved_tensors
        dmean, dpv = F_.latent_terms_backward_path(dz, mean, pv, eps, dlogpq, weights.s if weights.dreg else None)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None, None)


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


def rsample(z_vecs, W_mean: nn.Linear, W_var: nn.Linear, perturb: bool = True, z_width=None):
    """(z, kl) -- reference ggpm/property_vae.py:26-33. ``z_vecs`` may carry zero pad columns."""
    B, L = z_vecs.shape[0], W_mean.weight.shape[0]
    # the reference draws epsilon with torch's generator too
    eps = torch.randn(B, L, dtype=torch.float32, device=z_vecs.device) if perturb else None
    if W_mean.bias is None or W_var.bias is None:
        H = W_mean.weight.shape[1]
        z_mean = F_.linear([z_vecs], [H], W_mean.weight, W_mean.bias, ld_out=L)
        pre_var = F_.linear([z_vecs], [H], W_var.weight, W_var.bias, ld_out=L)
        return _RsampleTail.apply(z_mean, pre_var, eps)
    return _KLHead.apply(z_vecs, W_mean.weight, W_mean.bias, W_var.weight, W_var.bias, eps)


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

    def sample(self, batch_size, greedy=True, seed=None, max_decode_step=150, beam=5, graph_batch_factory=None):
        """New molecules from the prior (what reference ggpm/property_vae.py:35-37 intends): seeded standard-normal latents
        drawn on the device, then ``decode`` or, with ``greedy=False``, ``decode_sampled`` at the same seed ->
        (results, molecules)."""
        return _sample(self, batch_size, greedy, seed, max_decode_step, beam, graph_batch_factory)

    def log_likelihood(self, batch, n_samples=1, seed=None, sample_ids=None, eps=None, max_cls_size=None, schedule=None):
        """Per-molecule reconstruction terms, KL, ELBO and the ``n_samples``-sample importance-weighted bound of ``batch``
        (the tuple ``self(*batch)`` takes) -> :class:`MolLikelihood`; forward only, see :func:`log_likelihood`."""
        return log_likelihood(self, batch, n_samples, seed, sample_ids, eps, max_cls_size, schedule)

    def bound_loss(self, batch, n_samples=1, objective="elbo", beta=1.0, mol_weights=None, seed=None, sample_ids=None,
                   eps=None, max_cls_size=None, schedule=None, estimator="reparam", alpha=None, gamma=None, dataset_size=None,
                   free_bits=None):
        """The ``n_samples``-sample ELBO (``objective="elbo"``), importance-weighted bound (``"iwae"``) or beta-TCVAE loss
        (``"tcvae"``, with ``alpha``, ``gamma`` and ``dataset_size``) of ``batch`` as a loss to train on, with optional
        per-molecule weights, for the ELBO a free-bits KL and for the importance-weighted bound a choice of gradient
        estimator -> (loss, :class:`MolObjective`); see :func:`bound_loss`."""
        return bound_loss(self, batch, n_samples, objective, beta, mol_weights, seed, sample_ids, eps, max_cls_size, schedule,
                          estimator, alpha, gamma, dataset_size, free_bits)

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


def _sample(model, batch_size, greedy, seed, max_decode_step, beam, graph_batch_factory):
    """``sample`` of the four VAEs: [batch_size, decoder.latent_size] latents -- the width ``reconstruct`` hands to
    ``decode`` -- from ``functional.sample_normal`` (sample ids ``arange``), used as all three source vectors."""
    from .greedy_decode import split_seed
    dec = model.decoder
    factory = graph_batch_factory
    if factory is None:
        factory = _graph_batch_factory(model, getattr(model, "args", None))
    check_no_dropout(dec, "%s.sample runs without dropout: call model.eval() first" % type(model).__name__)
    if int(batch_size) < 1:
        raise ValueError("%s.sample: batch_size %d" % (type(model).__name__, batch_size))
    lo, hi = split_seed(seed)
    with torch.no_grad():
        z = F_.sample_normal(int(batch_size), dec.latent_size, lo, hi, device=next(dec.parameters()).device)
        if greedy:
            return dec.decode(None, (z, z, z), greedy=True, max_decode_step=max_decode_step, beam=beam,
                              graph_batch_factory=factory)
        return dec.decode_sampled(None, (z, z, z), seed=lo | hi << 32, max_decode_step=max_decode_step, beam=beam,
                                  graph_batch_factory=factory)


def _likelihood_args(model, what, batch, n_samples, sample_ids, eps, max_cls_size, schedule):
    """The argument checks ``log_likelihood`` and ``bound_loss`` share (``what``: the method's name in the messages) ->
    (class name, decoder, device, K, B, L, schedule, pinned max_cls_size)"""
    from .decoder import _pinned_cls_size
    name, dec = type(model).__name__, model.decoder
    check_no_dropout(model, "%s.%s runs without dropout: call model.eval() first" % (name, what), each_dropout=True)
    graphs, tensors, orders = batch[1], batch[2], batch[3]
    B, L = len(orders), model.R_mean.weight.shape[0]
    dev = model.R_mean.weight.device
    K = n_samples
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= F_.LIKELIHOOD_MAX_K:
        raise ValueError("%s.%s: n_samples %r (1 .. %d)" % (name, what, n_samples, F_.LIKELIHOOD_MAX_K))
    K = int(K)
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


def _likelihood_encode(model, what, tensors, schedule, record_grad):
    """What ``log_likelihood`` and ``bound_loss`` run once for all K draws, under the caller's grad mode: the atom level
    of the hierarchical decoder (``atom_level``, not the one posted beside the encoder) and the encoder ->
    (tensors on the device, atom, root vectors, stats)"""
    stats = dict(encoder_calls=0, atom_level_calls=0, decoder_passes=0)
    tensors = make_cuda(tensors)
    atom = None
    if model.HIER:
        atom = model.decoder.atom_level(schedule, tensors, record_grad=record_grad)
        if atom is None:
            raise NotImplementedError("%s.%s: this batch runs the decoder's step loop (no tree message at all, "
                                      "no AtomPlan, or a batched form switched off in ggpm_amd._dev), which has no "
                                      "per-molecule form" % (type(model).__name__, what))
        stats["atom_level_calls"] = 1
    root_vecs = model._encode(tensors)
    stats["encoder_calls"] = 1
    return tensors, atom, root_vecs, stats


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


def log_likelihood(model, batch, n_samples=1, seed=None, sample_ids=None, eps=None, max_cls_size=None, schedule=None):
    """``log_likelihood`` of the four VAEs (*Per-molecule ELBO and the importance-weighted bound*).

    The encoder, ``R_mean`` / ``R_var`` and -- for the hierarchical decoder -- the atom level run once: under teacher
    forcing none of them depends on the latent draw.  Per sample only ``z_k``, ``W_root``, the tree-side levels and the
    heads run.  ``eps[k, i, :]`` comes from the seeded stream of csrc/sample.hip at site LATENT, keyed by ``seed`` (an int,
    64 bits used; None takes them from torch's default CPU generator), ``sample_ids[i]`` (default ``arange``) and the counter
    ``k * L + column``: a molecule's draws do not depend on its batch, and the first K draws of a larger call are the
    K-sample call's.  ``eps=`` (a fp32 [K, B, L] tensor on the model's device, ``n_samples`` = K) replaces the stream; all
    zeros with K = 1 is the ``perturb_z=False`` latent.  ``max_cls_size``: see ``molecule_losses`` -- None is the training
    convention (the parts then add up to the training loss x B), an int makes numbers comparable across batches."""
    from .greedy_decode import split_seed
    name, dec, dev, K, B, L, schedule, C = _likelihood_args(model, "log_likelihood", batch, n_samples, sample_ids, eps,
                                                            max_cls_size, schedule)
    mols, graphs, tensors, orders = batch[0], batch[1], batch[2], batch[3]
    with torch.no_grad():
        tensors, atom, root_vecs, stats = _likelihood_encode(model, "log_likelihood", tensors, schedule, record_grad=False)
        Rm, Rv = model.R_mean, model.R_var
        mean, pre_var = _latent_heads(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias)
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
        elbo, iwae = F_.iwae_finish(parts, logpq, kl)
    return MolLikelihood(parts, kl, elbo, iwae, z, stats)


MolObjective = namedtuple("MolObjective", ["parts", "kl", "elbo", "iwae", "z", "weights", "stats"])
MolObjective.__doc__ = """The second value of ``bound_loss``: detached fp32 device tensors, the fields of :class:`MolLikelihood` (bit for
bit what ``log_likelihood`` returns for the same draws) plus ``weights [B]``, the molecule weights used (ones for None)."""


class FreeBitsObjective(MolObjective):
    """The second value of ``bound_loss(free_bits=...)``: :class:`MolObjective`'s seven fields (so unpacking it is unchanged)
    and two attributes, ``kl_dims`` (fp32 [L] on the device: klbar_j, the weighted batch mean of every latent column's KL)
    and ``free_bits`` (the float used)."""

    def __new__(cls, *fields, kl_dims, free_bits):
        self = super().__new__(cls, *fields)
        self.kl_dims, self.free_bits = kl_dims, free_bits
        return self


class EstimatorObjective(MolObjective):
    """The second value of ``bound_loss(objective="iwae", estimator="stl" | "dreg")``: :class:`MolObjective`'s seven fields
    (bit-equal to the ``estimator="reparam"`` call's) and three attributes, ``estimator`` (the name used), ``sample_weights``
    (fp32 [K, B] on the device: the normalised importance weights of every molecule's K samples) and ``ess`` (fp32 [B]: the
    effective sample size 1 / sum_k sample_weights^2, between 1 and K); the two tensors are detached."""

    def __new__(cls, *fields, estimator, sample_weights, ess):
        self = super().__new__(cls, *fields)
        self.estimator, self.sample_weights, self.ess = estimator, sample_weights, ess
        return self


class DecompositionObjective(MolObjective):
    """The second value of ``bound_loss(objective="tcvae")``: :class:`MolObjective`'s seven fields (bit-equal to the
    ``objective="elbo"`` call's on the same draws) and the attributes ``mi``, ``tc``, ``dwkl`` (fp32 [K, B] on the device,
    detached: the index-code mutual information, the total correlation and the dimension-wise KL of every draw), ``alpha``,
    ``beta``, ``gamma`` (the floats that weighed them) and ``dataset_size`` (the int used)."""

    def __new__(cls, *fields, mi, tc, dwkl, alpha, beta, gamma, dataset_size):
        self = super().__new__(cls, *fields)
        self.mi, self.tc, self.dwkl = mi, tc, dwkl
        self.alpha, self.beta, self.gamma, self.dataset_size = alpha, beta, gamma, dataset_size
        return self


ESTIMATORS = ("reparam", "stl", "dreg")


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
        self._check()
        Rm = model.R_mean.weight
        self.acc = torch.zeros(F_.LATENT_STAT_ROWS, Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.n_molecules = 0

    def _check(self):
        check_no_dropout(self.model, "%s.latent_stats runs without dropout: call model.eval() first"
                         % type(self.model).__name__, each_dropout=True)

    def update(self, batch):
        """Adds the molecules of ``batch`` (the tuple ``model(*batch)`` takes; only ``batch[2]``, the tensors, is used)."""
        self._check()
        model = self.model
        with torch.no_grad():
            root_vecs = model._encode(make_cuda(batch[2]))
            Rm, Rv = model.R_mean, model.R_var
            mean, pre_var = _latent_heads(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias)
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
        self._check()
        F_.latent_decomp_log_nb("%s.latent_decomposition" % name, dataset_size, 1)
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= int(n_samples) <= F_.LIKELIHOOD_MAX_K:
            raise ValueError("%s.latent_decomposition: n_samples %r (1 .. %d)" % (name, n_samples, F_.LIKELIHOOD_MAX_K))
        self.dataset_size, self.n_samples = dataset_size, int(n_samples)
        self.seed = split_seed(seed)
        Rm = model.R_mean.weight
        self.acc = torch.zeros(F_.LATENT_DECOMP_ROWS + Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.dims = torch.zeros(F_.LATENT_STAT_ROWS, Rm.shape[0], dtype=torch.float64, device=Rm.device)
        self.n_molecules = 0

    def _check(self):
        check_no_dropout(self.model, "%s.latent_decomposition runs without dropout: call model.eval() first"
                         % type(self.model).__name__, each_dropout=True)

    def update(self, batch):
        """Adds the molecules of ``batch`` (the tuple ``model(*batch)`` takes; only ``batch[2]``, the tensors, is used)."""
        self._check()
        model = self.model
        with torch.no_grad():
            root_vecs = model._encode(make_cuda(batch[2]))
            Rm, Rv = model.R_mean, model.R_var
            mean, pre_var = _latent_heads(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias)
            B, L = mean.shape
            F_.latent_decomp_log_nb("%s.latent_decomposition" % type(model).__name__, self.dataset_size, B)
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


def bound_loss(model, batch, n_samples=1, objective="elbo", beta=1.0, mol_weights=None, seed=None, sample_ids=None, eps=None,
               max_cls_size=None, schedule=None, estimator="reparam", alpha=None, gamma=None, dataset_size=None, free_bits=None):
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
    ``estimator``, ``sample_weights`` ([K, B]) and ``ess`` ([B])."""
    from .greedy_decode import split_seed
    name, dec, dev, K, B, L, schedule, C = _likelihood_args(model, "bound_loss", batch, n_samples, sample_ids, eps,
                                                            max_cls_size, schedule)
    if objective not in F_.BOUND_OBJECTIVES and objective != "tcvae":
        raise ValueError("%s.bound_loss: objective %r (one of %s)" % (name, objective, sorted(F_.BOUND_OBJECTIVES) + ["tcvae"]))
    if estimator not in ESTIMATORS:
        raise ValueError("%s.bound_loss: estimator %r (one of %s)" % (name, estimator, ", ".join(ESTIMATORS)))
    if estimator != "reparam" and objective != "iwae":
        raise ValueError("%s.bound_loss: estimator %r changes the gradient of the importance-weighted bound; objective %r has "
                         "an analytic KL and no score term to remove (free_bits included)" % (name, estimator, objective))
    tcvae = objective == "tcvae"
    if not tcvae and (alpha is not None or gamma is not None or dataset_size is not None):
        raise ValueError("%s.bound_loss: alpha, gamma and dataset_size weigh the split KL of objective \"tcvae\"; objective %r "
                         "has none" % (name, objective))
    if tcvae:
        if estimator != "reparam":
            raise ValueError("%s.bound_loss: estimator %r changes the gradient of the importance-weighted bound; objective "
                             "\"tcvae\" takes \"reparam\"" % (name, estimator))
        if free_bits is not None:
            raise ValueError("%s.bound_loss: free_bits holds the KL of the ELBO; objective \"tcvae\" splits it instead" % name)
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
    beta = float(beta)
    if objective == "iwae" and beta != 1.0:
        raise ValueError("%s.bound_loss: the importance-weighted bound has no beta (got %r): pass beta=1.0" % (name, beta))
    if free_bits is not None:
        if objective != "elbo":
            raise ValueError("%s.bound_loss: free_bits holds the KL of the ELBO; objective %r has none to hold" % (name, objective))
        free_bits = float(free_bits)
        if not (0.0 <= free_bits < float("inf")):
            raise ValueError("%s.bound_loss: free_bits %r (None, or a finite value >= 0)" % (name, free_bits))
        if L > F_.FREE_BITS_MAX_L:
            raise ValueError("%s.bound_loss: free_bits for %d latent columns (at most %d)" % (name, L, F_.FREE_BITS_MAX_L))
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
    mols, graphs, tensors, orders = batch[0], batch[1], batch[2], batch[3]
    with torch.enable_grad():
        tensors, atom, root_vecs, stats = _likelihood_encode(model, "bound_loss", tensors, schedule, record_grad=True)
        if eps is None:
            lo, hi = split_seed(seed)
            eps = F_.sample_latent_normal(K, B, L, lo, hi, ids=sample_ids, device=dev)
        Rm, Rv = model.R_mean, model.R_var
        weights = None
        if estimator != "reparam":
            weights = _ImportanceWeights(dreg=estimator == "dreg")
            z, kl, logpq = _PathLatentTerms.apply(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias, eps.detach(), weights)
        elif tcvae:
            z, kl, logpq, comps = _DecompLatentTerms.apply(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias, eps.detach(),
                                                           dataset_size)
        elif free_bits is None:
            z, kl, logpq = _LatentTerms.apply(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias, eps.detach())
        else:
            z, kl, logpq, term, kl_dims = _FreeBitsLatentTerms.apply(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias,
                                                                     eps.detach(), w, free_bits)
        parts = []
        for k in range(K):
            zk = z[k]
            parts.append(dec.molecule_losses(mols, (zk, zk, zk), graphs, tensors, orders, schedule=schedule, max_cls_size=C,
                                             atom=atom))
            stats["decoder_passes"] += 1
        parts = torch.stack(parts, dim=0)
        if weights is not None:
            with torch.no_grad():
                weights.s, weights.ess = F_.iwae_weights(parts.detach(), logpq.detach())
        if tcvae:
            # the reconstruction part is the ELBO without its KL; the three components join it as one weighted sum (formed in
            # fp64: tc and dwkl carry +- L log(N B), which cancels between them)
            cw = (torch.ones(B, dtype=torch.float64, device=dev) if w is None else w.double()) / float(B * K)
            cw = cw[None, :, None] * torch.tensor([alpha, beta, gamma], dtype=torch.float64, device=dev)
            loss = _BoundObjective.apply(parts, logpq, kl, w, "elbo", 0.0, tuple(model.parameters())) + \
                (comps.double() * cw).sum().to(torch.float32)
        elif free_bits is None:
            loss = _BoundObjective.apply(parts, logpq, kl, w, objective, beta, tuple(model.parameters()))
        else:
            # the reconstruction part is the ELBO without its KL; the held KL joins it as one term
            loss = _BoundObjective.apply(parts, logpq, kl, w, objective, 0.0, tuple(model.parameters())) + beta * term
    with torch.no_grad():
        elbo, iwae = F_.iwae_finish(parts.detach(), logpq.detach(), kl.detach())
    ones = w if w is not None else torch.ones(B, dtype=torch.float32, device=dev)
    fields = (parts.detach(), kl.detach(), elbo, iwae, z.detach(), ones, stats)
    if tcvae:
        c = comps.detach()
        return loss, DecompositionObjective(*fields, mi=c[..., 0], tc=c[..., 1], dwkl=c[..., 2], alpha=alpha, beta=beta,
                                            gamma=gamma, dataset_size=dataset_size)
    if weights is not None:
        return loss, EstimatorObjective(*fields, estimator=estimator, sample_weights=weights.s, ess=weights.ess)
    if free_bits is None:
        return loss, MolObjective(*fields)
    return loss, FreeBitsObjective(*fields, kl_dims=kl_dims.detach(), free_bits=free_bits)


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
