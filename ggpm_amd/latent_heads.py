"""The latent heads ``R_mean`` / ``R_var`` of the four VAEs: ``rsample`` (reference ggpm/property_vae.py:26-33) and its form
for K draws, the latent-terms node of ``bound_loss``.  The two [B,H]x[H,latent] products run through the library GEMM, the
[B,latent] elementwise tail (|.|, exp, KL sum, reparameterisation) is one HIP launch each way (csrc/losses.hip)."""
import torch
import torch.nn as nn

from . import _lib, functional as F_


def _rsample_forward(mean, pv, eps):
    """(mean, pv [B, L], eps [B, L] or None) -> (z [B, L], kl 0-dim): the elementwise tail of rsample, one launch"""
    B, L = mean.shape
    z = torch.empty_like(mean)
    kl = torch.empty(1, dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().ggpm_rsample_forward(F_._p(mean), F_._p(pv), F_._p(eps), B, L, F_._p(z), F_._p(kl),
                                                F_._stream()), "rsample_forward")
    return z, kl.reshape(())


def _rsample_backward(mean, pv, eps, dz, dkl):
    """The gradients that reached (z, kl), None for zeros -> (dmean, dpv): the tail's way back, one launch"""
    B, L = mean.shape
    dz = dz.contiguous() if dz is not None else None
    dkl = dkl.reshape(1).contiguous() if dkl is not None else None
    dmean, dpv = torch.empty_like(mean), torch.empty_like(pv)
    _lib.check(_lib.load().ggpm_rsample_backward(F_._p(mean), F_._p(pv), F_._p(eps), F_._p(dz), F_._p(dkl), B, L,
                                                 F_._p(dmean), F_._p(dpv), F_._stream()), "rsample_backward")
    return dmean, dpv


class _RsampleTail(torch.autograd.Function):
    """(mean, pv, eps) -> (z, kl): the elementwise part of rsample in one launch each way (csrc/losses.hip)."""

    @staticmethod
    def forward(ctx, mean, pv, eps):
        mean, pv, eps = mean.contiguous(), pv.contiguous(), eps.contiguous() if eps is not None else None
        ctx.save_for_backward(mean, pv)
        ctx.eps = eps
        return _rsample_forward(mean, pv, eps)

    @staticmethod
    def backward(ctx, dz, dkl):
        mean, pv = ctx.saved_tensors
        return _rsample_backward(mean, pv, ctx.eps, dz, dkl) + (None,)


def _latent_heads(z_vecs, Wm, bm, Wv, bv):
    """(mean, pre_var) = (R_mean(h), R_var(h)): both [B,H]x[H,latent] products in one grouped launch"""
    B, (L, H) = z_vecs.shape[0], Wm.shape
    mean = torch.empty(B, L, dtype=torch.float32, device=z_vecs.device)
    pv = torch.empty(B, L, dtype=torch.float32, device=z_vecs.device)
    F_.gemm_grouped(0, 1, B, L, H, [
        dict(A=z_vecs, lda=F_._ld(z_vecs), B=Wm, ldb=Wm.stride(0), C=mean, ldc=L, n_pad=L, bias=bm),
        dict(A=z_vecs, lda=F_._ld(z_vecs), B=Wv, ldb=Wv.stride(0), C=pv, ldc=L, n_pad=L, bias=bv)])
    return mean, pv


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
        F_.publish_aside(z_vecs.device, (dmean, dpv, z_vecs), ctx.params, param_grads)
        return dx, None, None, None, None
    dWm, dbm, dWv, dbv = param_grads()
    return dx, dWm, dbm, dWv, dbv


class _KLHead(torch.autograd.Function):
    """The whole of rsample as ONE autograd node: both [B,H]x[H,latent] products in one grouped launch, the elementwise
    tail in one launch, and on the way back one launch for d(z_vecs) (two K segments), one grouped launch for the two
    weight gradients (second stream, straight into ``.grad`` like the level functions do)."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv)
        ctx.eps = eps
        ctx.params = (Wm, bm, Wv, bv)           # the Parameter objects themselves (their .grad is assigned)
        return _rsample_forward(mean, pv, eps)

    @staticmethod
    def backward(ctx, dz, dkl):
        z_vecs, Wm, Wv, mean, pv = ctx.saved_tensors
        dmean, dpv = _rsample_backward(mean, pv, ctx.eps, dz, dkl)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None,)


class Plain:
    """What ``_LatentTerms`` computes beside (z, kl, logpq): nothing.  A variant of the node overrides ``extras`` (further
    outputs and the tensors their backward needs) and ``backward`` (what happens around ggpm_latent_terms_backward); the
    variants of ``bound_loss`` are in objectives.py."""

    def extras(self, ctx, z, mean, pv):
        """-> (further outputs of the node behind z, kl, logpq; further tensors to save behind the node's six)"""
        return (), ()

    def backward(self, dz, dkl, dlogpq, dextras, mean, pv, eps, saved):
        """The gradients that reached z, kl, logpq and the further outputs (None: none did) and what ``extras`` saved ->
        (dmean, dpre_var): ggpm_latent_terms_backward (the K gradients of z, of logpq and of kl summed in a fixed order)"""
        return F_.latent_terms_backward(dz, mean, pv, eps, dlogpq, dkl)


class _LatentTerms(torch.autograd.Function):
    """_KLHead for K draws per molecule: (z_vecs, R_mean, R_var, eps [K, B, L]) -> (z [K, B, L], kl [B], logpq [K, B]) and
    the further outputs of ``variant`` -- ``_latent_heads`` and ggpm_latent_terms, the launches of ``log_likelihood`` -- and
    on the way back the variant's backward (for ``Plain`` ggpm_latent_terms_backward), then _KLHead's tail.  Gradients that
    did not arrive stay None down to the kernels, which take null for zeros."""

    @staticmethod
    def forward(ctx, z_vecs, Wm, bm, Wv, bv, eps, variant=Plain()):
        mean, pv = _latent_heads(z_vecs, Wm, bm, Wv, bv)
        z, kl, logpq = F_.latent_terms(mean, pv, eps)
        outputs, saved = variant.extras(ctx, z, mean, pv)
        ctx.save_for_backward(z_vecs, Wm, Wv, mean, pv, eps, *saved)
        ctx.params = (Wm, bm, Wv, bv)
        ctx.variant = variant
        ctx.set_materialize_grads(False)
        return (z, kl, logpq) + outputs

    @staticmethod
    def backward(ctx, dz, dkl, dlogpq, *dextras):
        z_vecs, Wm, Wv, mean, pv, eps, *saved = ctx.saved_tensors
        dmean, dpv = ctx.variant.backward(dz, dkl, dlogpq, dextras, mean, pv, eps, saved)
        return _latent_heads_backward(ctx, z_vecs, Wm, Wv, dmean, dpv) + (None, None)


def _encode_heads(model, tensors):
    """(root vectors, mean, pre_var) of ``tensors`` (on the device): the model's encoder, then its latent heads, under the
    caller's grad mode"""
    root_vecs = model._encode(tensors)
    Rm, Rv = model.R_mean, model.R_var
    return (root_vecs,) + _latent_heads(root_vecs, Rm.weight, Rm.bias, Rv.weight, Rv.bias)


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
