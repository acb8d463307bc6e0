"""A learnable prior for the four VAEs: ``MixturePrior``, a mixture of diagonal Gaussians with learnable weights, means and
variances (*A learned prior*).  The density, its gradient and the sampler are the three entries of
csrc/latent_prior.hip; this module is their autograd node and the ``nn.Module`` that owns the three parameters.  The prior
is a module of its own: it is not part of a model's ``state_dict`` nor of the flat buffers of parallel.FlatGradSync /
optim.FlatAdam -- give its three tensors to a torch optimizer."""
import numpy as np
import torch
import torch.nn as nn

from . import functional as F_

SITE_PRIOR_COMP = 260           # include/ggpm_hip.h GGPM_SITE_SAMPLE_PRIOR_COMP


class _MixtureLogp(torch.autograd.Function):
    """(z [..., L], logits, means, log_vars) -> log p(z) (``on_logp``) or log p(z) - log N(z; 0, I), [...]: ggpm_mixture_logp,
    and on the way back ggpm_mixture_logp_backward -- the row pass only where z asks for a gradient, the column pass only
    where a parameter does.  ``count``: called with the number of launches issued, each way."""

    @staticmethod
    def forward(ctx, z, logits, means, log_vars, on_logp, count):
        z2 = z.reshape(-1, z.shape[-1]).contiguous()
        logp, ratio, _, comp_stash, logp_stash = F_.mixture_logp(z2, logits, means, log_vars)
        ctx.save_for_backward(z2, logits, means, log_vars)
        ctx.stash, ctx.on_logp, ctx.count, ctx.z_shape = (comp_stash, logp_stash), on_logp, count, z.shape
        count(1)
        return (logp if on_logp else ratio).reshape(z.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        if ctx.stash is None:
            raise F_.second_backward("mixture prior")
        (comp_stash, logp_stash), ctx.stash = ctx.stash, None
        z2, logits, means, log_vars = ctx.saved_tensors
        want_dz, want_params = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:4])
        if not want_dz and not want_params:
            return (None,) * 6
        dz, dm, ds, da = F_.mixture_logp_backward(z2, logits, means, log_vars, comp_stash, logp_stash,
                                                  g.reshape(-1).to(torch.float32), ctx.on_logp, want_dz, want_params)
        ctx.count(int(want_dz) + int(want_params))
        return (dz.reshape(ctx.z_shape) if want_dz else None), da, dm, ds, None, None


def _no_count(n):
    pass


def _stream_words(seed_lo, seed_hi, site, ids, step, slot):
    """m(site, id, step, slot) of the seeded stream (include/ggpm_hip.h) on the host -> uint64 array of 24-bit words"""
    M = np.uint64(0xFFFFFFFF)

    def mix(h):
        h = h & M
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x85EBCA6B)) & M
        h ^= h >> np.uint64(13)
        h = (h * np.uint64(0xC2B2AE35)) & M
        return h ^ (h >> np.uint64(16))

    ids = np.asarray(ids, np.uint64) & M
    base = mix(mix(ids * np.uint64(0x9E3779B1) + np.uint64(seed_lo)) ^ ((np.uint64(seed_hi) + np.uint64(site * 0x7F4A7C15 & 0xFFFFFFFF)) & M))
    ctr = np.uint64((step * 64 + slot) * 0x9E3779B1 & 0xFFFFFFFF)
    return mix(base + ctr) >> np.uint64(8)


class MixturePrior(nn.Module):
    """p(z) = sum_c pi_c N(z; m_c, diag(exp(s_c))), pi = softmax(logits): ``logits`` [C], ``means`` [C, L], ``log_vars``
    [C, L], fp32 parameters.  The default initialisation draws the means from N(0, init_std^2) with torch's generator
    (``torch.manual_seed`` makes it reproducible) and sets ``log_vars`` and ``logits`` to 0.  Everything that computes runs on
    the MI355X; with the parameters on the CPU the methods raise."""

    def __init__(self, n_components, latent_size, init_std=1.0):
        super().__init__()
        for what, v, top in (("n_components", n_components, F_.MIXTURE_MAX_C), ("latent_size", latent_size, F_.FREE_BITS_MAX_L)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
                raise ValueError("MixturePrior: %s %r (an int in 1 .. %d)" % (what, v, top))
        init_std = float(init_std)
        if not (0.0 <= init_std < float("inf")):
            raise ValueError("MixturePrior: init_std %r (a finite value >= 0)" % init_std)
        self.n_components, self.latent_size = n_components, latent_size
        self.logits = nn.Parameter(torch.zeros(n_components, dtype=torch.float32))
        self.means = nn.Parameter(torch.randn(n_components, latent_size, dtype=torch.float32) * init_std)
        self.log_vars = nn.Parameter(torch.zeros(n_components, latent_size, dtype=torch.float32))

    @classmethod
    def standard(cls, latent_size):
        """the one-component N(0, I): the prior the models assume without one"""
        return cls(1, latent_size, init_std=0.0)

    def _check_z(self, what, z):
        if not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or z.dim() < 1 or z.shape[-1] != self.latent_size or \
                z.numel() == 0:
            raise ValueError("MixturePrior.%s: z must be a non-empty float32 [..., %d] tensor, got %s"
                             % (what, self.latent_size, tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__))
        F_._need_gpu(z, self.means)
        if z.device != self.means.device:
            raise ValueError("MixturePrior.%s: z on %s, the prior on %s" % (what, z.device, self.means.device))

    def _logp(self, what, z, on_logp, count):
        self._check_z(what, z)
        count = count or _no_count
        if torch.is_grad_enabled() and any(t.requires_grad for t in (z, self.logits, self.means, self.log_vars)):
            return _MixtureLogp.apply(z, self.logits, self.means, self.log_vars, on_logp, count)
        logp, ratio = F_.mixture_logp(z.reshape(-1, self.latent_size), self.logits, self.means, self.log_vars, want_stash=False)[:2]
        count(1)
        return (logp if on_logp else ratio).reshape(z.shape[:-1])

    def log_prob(self, z, count=None):
        """log p(z) of ``z`` [..., L] (fp32, on the device) -> [...]; differentiable in z and in the three parameters"""
        return self._logp("log_prob", z, True, count)

    def log_ratio(self, z, count=None):
        """log p(z) - log N(z; 0, I) of ``z`` [..., L] -> [...], the difference formed in fp64 before its rounding: what the
        objectives add to the standard-normal terms.  ``count``: called with the number of launches issued, each way"""
        return self._logp("log_ratio", z, False, count)

    def responsibilities(self, z):
        """p(c | z) of ``z`` [..., L] -> [..., C]; no gradient"""
        self._check_z("responsibilities", z)
        with torch.no_grad():
            z2 = z.detach().reshape(-1, self.latent_size)
            resp = F_.mixture_logp(z2, self.logits, self.means, self.log_vars, want_resp=True, want_stash=False)[2]
        return resp.reshape(z.shape[:-1] + (self.n_components,))

    def sample(self, n, seed=None, sample_ids=None, return_components=False):
        """``n`` draws [n, L] on the device from the seeded stream: row r depends on ``seed`` (``split_seed``'s handling: an
        int, 64 bits used; None takes them from torch's default CPU generator), ``sample_ids[r]`` (default ``arange``) and
        the column only.  ``return_components``: -> (z, the int32 [n] component of every row)"""
        from .greedy_decode import split_seed
        if isinstance(n, bool) or int(n) != n or int(n) < 1:
            raise ValueError("MixturePrior.sample: n %r (an int >= 1)" % (n,))
        F_._need_gpu(self.means)
        lo, hi = split_seed(seed)
        with torch.no_grad():
            z, comp = F_.sample_mixture(self.logits, self.means, self.log_vars, int(n), lo, hi, ids=sample_ids,
                                        want_components=return_components)
        return (z, comp) if return_components else z

    def init_from_latents(self, z_or_means, seed=None):
        """Starts a fit from data: the means become C of the N rows of ``z_or_means`` [N, L] (latents or posterior means, on
        any device), chosen without replacement by the seeded stream -- the C rows with the smallest words of site
        PRIOR_COMP at step 1, keyed by the row's index --, every component's ``log_vars`` the log of the columns' variances
        over the N rows, and the logits 0.  Host arithmetic; no kernel."""
        from .greedy_decode import split_seed
        x = z_or_means
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.latent_size or x.shape[0] < max(self.n_components, 2):
            raise ValueError("MixturePrior.init_from_latents: a [N, %d] tensor with N >= %d rows, got %s"
                             % (self.latent_size, max(self.n_components, 2), tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__))
        lo, hi = split_seed(seed)
        x = x.detach().to(torch.float64).cpu()
        words = _stream_words(lo, hi, SITE_PRIOR_COMP, np.arange(x.shape[0]), 1, 0)
        rows = torch.from_numpy(np.argsort(words, kind="stable")[:self.n_components].copy())
        var = x.var(dim=0, unbiased=False).clamp_min(1e-12)
        with torch.no_grad():
            self.means.copy_(x[rows].to(torch.float32))
            self.log_vars.copy_(var.log().to(torch.float32).expand_as(self.log_vars))
            self.logits.zero_()
        return self


def check_prior(what, prior, latent_size, device):
    """``prior=`` of the models' methods: None, or a MixturePrior of the decoder's latent width on the model's device"""
    if prior is None:
        return None
    if not isinstance(prior, MixturePrior):
        raise ValueError("%s: prior must be a MixturePrior or None, got %s" % (what, type(prior).__name__))
    if prior.latent_size != latent_size:
        raise ValueError("%s: the prior is over %d latent columns, the model's latent has %d" % (what, prior.latent_size, latent_size))
    if prior.means.device != torch.device(device):
        raise ValueError("%s: the prior is on %s, the model on %s" % (what, prior.means.device, device))
    return prior
