"""torch.autograd wrappers over the C ABI (include/ggpm_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the stream and the autograd tape;
every number on the hot path is produced by a hand-written HIP kernel from libggpm_hip.so.  There is no CPU
or eager fallback: on a tensor that is not on a ROCm device these functions raise.

Conventions: feature matrices are 2-D fp32 tensors whose row stride may exceed the logical width; pad
columns are zero.  Index tensors are int32 (CSR) unless stated.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import List, Optional, Sequence, Tuple

import torch

from . import _dev, _lib
from .nnutils import version_of
from .parallel import grad_view

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3


def _stream() -> ctypes.c_void_p:
    # raw handle of torch's current stream on the current device (torch.cuda.current_stream() builds a Python
    # Stream object: ~9 us per call, and a step makes ~1000 of them)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ggpm_amd: tensors must live on the MI355X (got a %s tensor); there is no CPU path"
                               % t.device.type)


def sample_normal(rows: int, cols: int, seed_lo: int, seed_hi: int, ids=None, device=None, ld: Optional[int] = None):
    """[rows, cols] standard normals of the seeded stream (csrc/sample.hip, site PRIOR), row r keyed by ``ids[r]``
    (default ``arange``): a row's values depend on its id, the column and the seed only"""
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("ggpm_amd: sample_normal runs on the MI355X (got device %s); there is no CPU path" % dev)
    ids = torch.arange(rows, dtype=torch.int32) if ids is None else torch.as_tensor(ids).to(torch.int64).bitwise_and(
        0xFFFFFFFF).to(torch.int32)
    if ids.shape != (rows,):
        raise ValueError("sample_normal: %d ids for %d rows" % (ids.numel(), rows))
    out = torch.zeros(rows, cols if ld is None else ld, device=dev)
    ids = ids.to(dev)
    _lib.check(_lib.load().ggpm_sample_normal(_p(out), rows, cols, out.stride(0), _p(ids), seed_lo & 0xFFFFFFFF,
                                              seed_hi & 0xFFFFFFFF, _stream()), "sample_normal")
    return out[:, :cols]


LIKELIHOOD_MAX_K = 1024         # include/ggpm_hip.h GGPM_LIKELIHOOD_MAX_K


def sample_latent_normal(K: int, B: int, L: int, seed_lo: int, seed_hi: int, ids=None, device=None):
    """[K, B, L] standard normals of the seeded stream (csrc/sample.hip, site LATENT): element (k, b, c) is keyed by the
    seed, ``ids[b]`` (default ``arange``) and the counter ``k * L + c`` -- not by B, K or the molecule's place in the batch"""
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("ggpm_amd: sample_latent_normal runs on the MI355X (got device %s); there is no CPU path" % dev)
    ids = torch.arange(B, dtype=torch.int32) if ids is None else torch.as_tensor(ids).to(torch.int64).bitwise_and(
        0xFFFFFFFF).to(torch.int32)
    if ids.shape != (B,):
        raise ValueError("sample_latent_normal: %d ids for %d molecules" % (ids.numel(), B))
    out = torch.empty(K, B, L, dtype=torch.float32, device=dev)
    ids = ids.to(dev)
    _lib.check(_lib.load().ggpm_sample_latent_normal(_p(out), K, B, L, _p(ids), seed_lo & 0xFFFFFFFF, seed_hi & 0xFFFFFFFF,
                                                     _stream()), "sample_latent_normal")
    return out


class MolLossTerm(ctypes.Structure):
    """ggpm_mol_loss_term (include/ggpm_hip.h)"""
    _fields_ = [("row_loss", ctypes.c_void_p), ("mol", ctypes.c_void_p), ("stride", ctypes.c_int), ("n_rows", ctypes.c_int)]


def mol_loss_parts(terms, B: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``terms``: four entries ``(row_loss, mol, n_rows[, stride])`` or None (an absent term) -> parts [B, 4]: per molecule
    the sum of the row losses of each term (csrc/mol_loss.hip).  ``row_loss`` fp32, ``mol`` int32, both on the device."""
    if len(terms) != 4:
        raise ValueError("mol_loss_parts: four terms (topology, motif class, attachment class, attachment), got %d" % len(terms))
    arr = (MolLossTerm * 4)()
    dev = None
    for t, term in enumerate(terms):
        if term is None or term[2] == 0:
            continue
        v, mol, n = term[0], term[1], int(term[2])
        _need_gpu(v, mol)
        stride = int(term[3]) if len(term) > 3 else 1
        if v.dtype != torch.float32 or mol.dtype != torch.int32 or not mol.is_contiguous() or not v.is_contiguous():
            raise ValueError("mol_loss_parts: term %d needs contiguous fp32 row losses and a contiguous int32 row -> molecule "
                             "table" % t)
        if stride < 1 or mol.numel() < n or v.numel() < (n - 1) * stride + 1:
            raise ValueError("mol_loss_parts: term %d lists %d rows %d floats apart but holds %d losses and %d molecules"
                             % (t, n, stride, v.numel(), mol.numel()))
        arr[t] = MolLossTerm(v.data_ptr(), mol.data_ptr(), stride, n)
        dev = v.device
    if out is None:
        if dev is None:
            raise ValueError("mol_loss_parts: every term is absent and no output tensor names the device")
        out = torch.empty(B, 4, dtype=torch.float32, device=dev)
    elif out.shape != (B, 4) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("mol_loss_parts: out must be a contiguous fp32 [B, 4] tensor")
    _need_gpu(out)
    _lib.check(_lib.load().ggpm_mol_loss_parts(ctypes.byref(arr), B, _p(out), _stream()), "mol_loss_parts")
    return out


def latent_terms(mean: torch.Tensor, pre_var: torch.Tensor, eps: torch.Tensor):
    """mean, pre_var [B, L], eps [K, B, L] -> (z [K, B, L], kl [B], logpq [K, B]) (csrc/mol_loss.hip)"""
    _need_gpu(mean, pre_var, eps)
    K, B, L = eps.shape
    mean, pre_var, eps = mean.contiguous(), pre_var.contiguous(), eps.contiguous()
    if mean.shape != (B, L) or pre_var.shape != (B, L):
        raise ValueError("latent_terms: mean %s / pre_var %s for eps %s" % (tuple(mean.shape), tuple(pre_var.shape), (K, B, L)))
    f32 = dict(dtype=torch.float32, device=mean.device)
    z, kl, logpq = torch.empty(K, B, L, **f32), torch.empty(B, **f32), torch.empty(K, B, **f32)
    _lib.check(_lib.load().ggpm_latent_terms(_p(mean), _p(pre_var), _p(eps), K, B, L, _p(z), _p(kl), _p(logpq), _stream()),
               "latent_terms")
    return z, kl, logpq


def iwae_finish(parts: torch.Tensor, logpq: torch.Tensor, kl: torch.Tensor):
    """parts [K, B, 4], logpq [K, B], kl [B] -> (elbo [B], iwae [B]) (csrc/mol_loss.hip)"""
    _need_gpu(parts, logpq, kl)
    K, B = logpq.shape
    if parts.shape != (K, B, 4) or kl.shape != (B,):
        raise ValueError("iwae_finish: parts %s / kl %s for logpq %s" % (tuple(parts.shape), tuple(kl.shape), (K, B)))
    parts, logpq, kl = parts.contiguous(), logpq.contiguous(), kl.contiguous()
    f32 = dict(dtype=torch.float32, device=parts.device)
    elbo, iwae = torch.empty(B, **f32), torch.empty(B, **f32)
    _lib.check(_lib.load().ggpm_iwae_finish(_p(parts), _p(logpq), _p(kl), K, B, _p(elbo), _p(iwae), _stream()), "iwae_finish")
    return elbo, iwae


BOUND_OBJECTIVES = {"elbo": 0, "iwae": 1}       # include/ggpm_hip.h GGPM_BOUND_ELBO / GGPM_BOUND_IWAE


def bound_objective(parts: torch.Tensor, logpq: torch.Tensor, kl: torch.Tensor, w: Optional[torch.Tensor], objective: str,
                    beta: float):
    """parts [K, B, 4], logpq [K, B], kl [B], w [B] or None -> (loss [1], c_nll [K, B], c_logpq [K, B], c_kl [B]): the
    weighted K-sample ELBO / IWAE loss and its partial derivatives by nll, logpq and kl (csrc/mol_loss.hip)"""
    _need_gpu(parts, logpq, kl)
    K, B = logpq.shape
    if parts.shape != (K, B, 4) or kl.shape != (B,) or (w is not None and (w.shape != (B,) or w.dtype != torch.float32)):
        raise ValueError("bound_objective: parts %s / kl %s / w %s for logpq %s"
                         % (tuple(parts.shape), tuple(kl.shape), None if w is None else tuple(w.shape), (K, B)))
    if objective not in BOUND_OBJECTIVES:
        raise ValueError("bound_objective: objective %r (one of %s)" % (objective, sorted(BOUND_OBJECTIVES)))
    parts, logpq, kl = parts.contiguous(), logpq.contiguous(), kl.contiguous()
    w = w.contiguous() if w is not None else None
    f32 = dict(dtype=torch.float32, device=parts.device)
    loss, c_nll, c_logpq, c_kl = torch.empty(1, **f32), torch.empty(K, B, **f32), torch.empty(K, B, **f32), torch.empty(B, **f32)
    work = torch.empty(B, dtype=torch.float64, device=parts.device)
    _lib.check(_lib.load().ggpm_bound_objective(_p(parts), _p(logpq), _p(kl), _p(w), K, B, BOUND_OBJECTIVES[objective],
                                                float(beta), _p(work), _p(loss), _p(c_nll), _p(c_logpq), _p(c_kl), _stream()),
               "bound_objective")
    return loss, c_nll, c_logpq, c_kl


def scale_rows_by_mol(d: torch.Tensor, N: int, mol: torch.Tensor, coef: torch.Tensor, B: int,
                      g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d[m, 0:N] *= g[0] * coef[mol[m]] in place (csrc/mol_loss.hip); a row of no molecule in [0, B) becomes 0.  ``d`` fp32
    [M, ld >= N] or [M] with unit column stride, ``mol`` int32 [M], ``coef`` fp32 [B] (any stride, e.g. a column of [B, 4])."""
    _need_gpu(d, mol, coef)
    M = d.shape[0]
    ld = 1 if d.dim() == 1 else d.stride(0)
    if d.dtype != torch.float32 or (d.dim() == 2 and d.stride(1) != 1 and d.shape[1] > 1) or (d.dim() == 1 and M > 1 and d.stride(0) != 1):
        raise ValueError("scale_rows_by_mol: d must be fp32 rows with unit column stride")
    if mol.dtype != torch.int32 or not mol.is_contiguous() or mol.numel() < M or coef.dtype != torch.float32 or coef.shape != (B,):
        raise ValueError("scale_rows_by_mol: a contiguous int32 molecule per row and %d fp32 coefficients" % B)
    _lib.check(_lib.load().ggpm_scale_rows_by_mol(_p(d), ld, M, N, _p(mol), _p(coef), max(coef.stride(0), 1), B, _p(g),
                                                  _stream()), "scale_rows_by_mol")
    return d


def latent_terms_backward(dz: Optional[torch.Tensor], mean: torch.Tensor, pre_var: torch.Tensor, eps: torch.Tensor,
                          c_logpq: Optional[torch.Tensor], c_kl: Optional[torch.Tensor], g: Optional[torch.Tensor] = None):
    """The backward of ``latent_terms``: dz [K, B, L], the gradients that reached logpq [K, B] and kl [B] (each None for
    zeros) -> (dmean [B, L], dpre_var [B, L]) (csrc/mol_loss.hip)"""
    _need_gpu(mean, pre_var, eps)
    K, B, L = eps.shape
    cont = lambda t: t.contiguous() if t is not None else None
    dz, c_logpq, c_kl = cont(dz), cont(c_logpq), cont(c_kl)
    if mean.shape != (B, L) or pre_var.shape != (B, L) or (dz is not None and dz.shape != (K, B, L)) or \
            (c_logpq is not None and c_logpq.shape != (K, B)) or (c_kl is not None and c_kl.shape != (B,)):
        raise ValueError("latent_terms_backward: shapes do not fit eps %s" % ((K, B, L),))
    mean, pre_var, eps = mean.contiguous(), pre_var.contiguous(), eps.contiguous()
    dmean, dpv = torch.empty_like(mean), torch.empty_like(pre_var)
    _lib.check(_lib.load().ggpm_latent_terms_backward(_p(dz), _p(mean), _p(pre_var), _p(eps), _p(c_logpq), _p(c_kl), _p(g), K, B,
                                                      L, _p(dmean), _p(dpv), _stream()), "latent_terms_backward")
    return dmean, dpv


def _fp32(what: str, **named) -> None:
    for k, t in named.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise ValueError("%s: %s must be a float32 tensor" % (what, k))


def iwae_weights(parts: torch.Tensor, logpq: torch.Tensor):
    """parts [K, B, 4], logpq [K, B] -> (s [K, B]: the normalised importance weights softmax_k(logpq - nll), ess [B]: the
    effective sample size 1 / sum_k s^2 of every molecule) (csrc/mol_loss.hip)"""
    _fp32("iwae_weights", parts=parts, logpq=logpq)
    if logpq.dim() != 2 or logpq.numel() == 0 or parts.shape != (logpq.shape[0], logpq.shape[1], 4):
        raise ValueError("iwae_weights: parts %s for logpq %s ([K, B, 4] and [K, B])" % (tuple(parts.shape), tuple(logpq.shape)))
    _need_gpu(parts, logpq)
    K, B = logpq.shape
    parts, logpq = parts.contiguous(), logpq.contiguous()
    f32 = dict(dtype=torch.float32, device=parts.device)
    s, ess = torch.empty(K, B, **f32), torch.empty(B, **f32)
    _lib.check(_lib.load().ggpm_iwae_weights(_p(parts), _p(logpq), K, B, _p(s), _p(ess), _stream()), "iwae_weights")
    return s, ess


def latent_terms_backward_path(dz: Optional[torch.Tensor], mean: torch.Tensor, pre_var: torch.Tensor, eps: torch.Tensor,
                               c_logpq: Optional[torch.Tensor], s: Optional[torch.Tensor] = None,
                               g: Optional[torch.Tensor] = None):
    """``latent_terms_backward`` with the parameters of log q held fixed (the path derivative): dz [K, B, L] and the gradient
    that reached logpq [K, B] (each None for zeros), ``s`` [K, B] the normalised importance weights for the doubly
    reparameterised estimator or None for "sticking the landing", ``g`` fp32 [1] or None: 1 -> (dmean [B, L],
    dpre_var [B, L]) (csrc/mol_loss.hip)"""
    what = "latent_terms_backward_path"
    _fp32(what, dz=dz, mean=mean, pre_var=pre_var, eps=eps, c_logpq=c_logpq, s=s, g=g)
    if eps.dim() != 3 or eps.numel() == 0:
        raise ValueError("%s: eps %s must be [K, B, L]" % (what, tuple(eps.shape)))
    K, B, L = eps.shape
    if mean.shape != (B, L) or pre_var.shape != (B, L) or (dz is not None and dz.shape != (K, B, L)) or \
            (c_logpq is not None and c_logpq.shape != (K, B)) or (s is not None and s.shape != (K, B)):
        raise ValueError("%s: shapes do not fit eps %s" % (what, (K, B, L)))
    if g is not None and g.numel() != 1:
        raise ValueError("%s: g must hold one fp32 value" % what)
    _need_gpu(dz, mean, pre_var, eps, c_logpq, s, g)
    cont = lambda t: t.contiguous() if t is not None else None
    dz, c_logpq, s = cont(dz), cont(c_logpq), cont(s)
    mean, pre_var, eps = mean.contiguous(), pre_var.contiguous(), eps.contiguous()
    dmean, dpv = torch.empty_like(mean), torch.empty_like(pre_var)
    _lib.check(_lib.load().ggpm_latent_terms_backward_path(_p(dz), _p(mean), _p(pre_var), _p(eps), _p(c_logpq), _p(s), _p(g), K,
                                                           B, L, _p(dmean), _p(dpv), _stream()), what)
    return dmean, dpv


LATENT_STAT_ROWS = 5            # include/ggpm_hip.h GGPM_LATENT_STAT_ROWS / GGPM_LATENT_STAT_OUT
FREE_BITS_MAX_L = 4096          # include/ggpm_hip.h GGPM_FREE_BITS_MAX_L


def _latent_pair(what: str, mean: torch.Tensor, pre_var: torch.Tensor, w: Optional[torch.Tensor] = None):
    """the checks the per-dimension entries share -> (mean, pre_var, w) contiguous, B, L"""
    _need_gpu(mean, pre_var, w)
    if mean.dim() != 2 or pre_var.shape != mean.shape or mean.dtype != torch.float32 or pre_var.dtype != torch.float32 or \
            mean.numel() == 0:
        raise ValueError("%s: mean %s / pre_var %s must be fp32 [B, L] of one shape" % (what, tuple(mean.shape), tuple(pre_var.shape)))
    B, L = mean.shape
    if w is not None and (w.shape != (B,) or w.dtype != torch.float32):
        raise ValueError("%s: %s weights for %d molecules (fp32 [B])" % (what, tuple(w.shape), B))
    return mean.contiguous(), pre_var.contiguous(), (w.contiguous() if w is not None else None), B, L


def _free_bits_lambda(what: str, lam, L: int) -> float:
    lam = float(lam)
    if not (0.0 <= lam < float("inf")):
        raise ValueError("%s: lambda %r (a finite value >= 0)" % (what, lam))
    if L > FREE_BITS_MAX_L:
        raise ValueError("%s: %d latent columns (at most %d)" % (what, L, FREE_BITS_MAX_L))
    return lam


def latent_dim_accumulate(mean: torch.Tensor, pre_var: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """Adds the per-column sums of mean, pre_var [B, L] to ``acc``, a contiguous fp64 [5, L] device tensor the caller zeroed
    once (rows: count, sum mean, sum mean^2, sum exp(lv), sum kl_dim) -> acc (csrc/latent_dims.hip)"""
    mean, pre_var, _, B, L = _latent_pair("latent_dim_accumulate", mean, pre_var)
    _need_gpu(acc)
    if acc.shape != (LATENT_STAT_ROWS, L) or acc.dtype != torch.float64 or not acc.is_contiguous():
        raise ValueError("latent_dim_accumulate: acc must be a contiguous fp64 [%d, %d] tensor, got %s %s"
                         % (LATENT_STAT_ROWS, L, acc.dtype, tuple(acc.shape)))
    _lib.check(_lib.load().ggpm_latent_dim_accumulate(_p(mean), _p(pre_var), B, L, _p(acc), _stream()), "latent_dim_accumulate")
    return acc


def latent_dim_finish(acc: torch.Tensor, au_threshold: float = 0.01):
    """acc fp64 [5, L] -> (out fp32 [5, L]: kl_dims, mu_mean, mu_var, sigma2_mean, agg_var; n_active int32 [1]: the columns
    with mu_var > au_threshold) (csrc/latent_dims.hip)"""
    _need_gpu(acc)
    if acc.dim() != 2 or acc.shape[0] != LATENT_STAT_ROWS or acc.shape[1] < 1 or acc.dtype != torch.float64 or \
            not acc.is_contiguous():
        raise ValueError("latent_dim_finish: acc must be a contiguous fp64 [%d, L] tensor, got %s %s"
                         % (LATENT_STAT_ROWS, acc.dtype, tuple(acc.shape)))
    au_threshold = float(au_threshold)
    if au_threshold != au_threshold:
        raise ValueError("latent_dim_finish: au_threshold is NaN")
    L = acc.shape[1]
    out = torch.empty(LATENT_STAT_ROWS, L, dtype=torch.float32, device=acc.device)
    n_active = torch.empty(1, dtype=torch.int32, device=acc.device)
    _lib.check(_lib.load().ggpm_latent_dim_finish(_p(acc), L, au_threshold, _p(out), _p(n_active), _stream()), "latent_dim_finish")
    return out, n_active


def free_bits_kl(mean: torch.Tensor, pre_var: torch.Tensor, w: Optional[torch.Tensor], lam: float):
    """mean, pre_var [B, L], w [B] or None -> (kl_dims [L]: the batch-mean weighted KL of every latent column, term [1]:
    sum_j max(lam, kl_dims_j) formed in fp64) (csrc/latent_dims.hip)"""
    mean, pre_var, w, B, L = _latent_pair("free_bits_kl", mean, pre_var, w)
    lam = _free_bits_lambda("free_bits_kl", lam, L)
    f32 = dict(dtype=torch.float32, device=mean.device)
    kl_dims, term = torch.empty(L, **f32), torch.empty(1, **f32)
    _lib.check(_lib.load().ggpm_free_bits_kl(_p(mean), _p(pre_var), _p(w), B, L, lam, _p(kl_dims), _p(term), _stream()),
               "free_bits_kl")
    return kl_dims, term


def free_bits_kl_backward(mean: torch.Tensor, pre_var: torch.Tensor, w: Optional[torch.Tensor], lam: float,
                          g: Optional[torch.Tensor] = None, kl_dims: Optional[torch.Tensor] = None):
    """The gradient of ``free_bits_kl``'s term times ``g`` (fp32 [1] or None: 1) -> (dmean [B, L], dpre_var [B, L]), zero in
    the columns that are free.  ``kl_dims``: the forward's, which spares the columns it decides their sum; the result does
    not depend on it (csrc/latent_dims.hip)"""
    mean, pre_var, w, B, L = _latent_pair("free_bits_kl_backward", mean, pre_var, w)
    lam = _free_bits_lambda("free_bits_kl_backward", lam, L)
    _need_gpu(g, kl_dims)
    if g is not None and (g.numel() != 1 or g.dtype != torch.float32):
        raise ValueError("free_bits_kl_backward: g must hold one fp32 value")
    if kl_dims is not None and (kl_dims.shape != (L,) or kl_dims.dtype != torch.float32):
        raise ValueError("free_bits_kl_backward: kl_dims %s for %d latent columns (fp32 [L])" % (tuple(kl_dims.shape), L))
    kl_dims = kl_dims.contiguous() if kl_dims is not None else None
    dmean, dpv = torch.empty_like(mean), torch.empty_like(pre_var)
    _lib.check(_lib.load().ggpm_free_bits_kl_backward(_p(mean), _p(pre_var), _p(w), _p(kl_dims), B, L, lam, _p(g), _p(dmean),
                                                      _p(dpv), _stream()), "free_bits_kl_backward")
    return dmean, dpv


LATENT_DECOMP_ROWS = 4          # include/ggpm_hip.h GGPM_LATENT_DECOMP_ROWS
LATENT_DECOMP_MAX_B = 4096      # include/ggpm_hip.h GGPM_LATENT_DECOMP_MAX_B


def _decomp_args(what: str, z: torch.Tensor, mean: torch.Tensor, pre_var: torch.Tensor):
    """the checks the entries of the KL split share (no device needed for the ValueErrors) -> K, B, L"""
    _fp32(what, z=z, mean=mean, pre_var=pre_var)
    if z.dim() != 3 or z.numel() == 0 or mean.shape != z.shape[1:] or pre_var.shape != z.shape[1:]:
        raise ValueError("%s: z %s must be [K, B, L] and mean %s / pre_var %s [B, L]"
                         % (what, tuple(z.shape), tuple(mean.shape), tuple(pre_var.shape)))
    K, B, L = z.shape
    if K > LIKELIHOOD_MAX_K or B > LATENT_DECOMP_MAX_B or L > FREE_BITS_MAX_L or K * B * L >= 1 << 31:
        raise ValueError("%s: %d samples of %d molecules and %d latent columns (at most %d, %d and %d, fewer than 2^31 elements)"
                         % (what, K, B, L, LIKELIHOOD_MAX_K, LATENT_DECOMP_MAX_B, FREE_BITS_MAX_L))
    return K, B, L


def latent_decomp_log_nb(what: str, dataset_size, B: int) -> float:
    """log(N B) of minibatch-weighted sampling; ``dataset_size``: an int >= B"""
    if isinstance(dataset_size, bool) or not isinstance(dataset_size, int) or dataset_size < B:
        raise ValueError("%s: dataset_size %r (an int, at least the %d molecules of the batch)" % (what, dataset_size, B))
    import math
    return math.log(float(dataset_size) * float(B))


def latent_decomposition(z: torch.Tensor, mean: torch.Tensor, pre_var: torch.Tensor, dataset_size: int):
    """z [K, B, L] the draws, mean, pre_var [B, L] the posteriors, ``dataset_size`` N -> (comps fp32 [K, B, 3]: the index-code
    mutual information, the total correlation and the dimension-wise KL of every draw by minibatch-weighted sampling,
    dwkl_dim fp32 [K, B, L], lse_joint fp64 [K, B], lse_dim fp64 [K, B, L]: what the backward reads) (csrc/latent_decomp.hip)"""
    what = "latent_decomposition"
    K, B, L = _decomp_args(what, z, mean, pre_var)
    log_nb = latent_decomp_log_nb(what, dataset_size, B)
    _need_gpu(z, mean, pre_var)
    z, mean, pre_var = z.contiguous(), mean.contiguous(), pre_var.contiguous()
    dev = z.device
    comps = torch.empty(K, B, 3, dtype=torch.float32, device=dev)
    dwkl_dim = torch.empty(K, B, L, dtype=torch.float32, device=dev)
    lse_joint = torch.empty(K, B, dtype=torch.float64, device=dev)
    lse_dim = torch.empty(K, B, L, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().ggpm_latent_decomp(_p(z), _p(mean), _p(pre_var), K, B, L, log_nb, _p(comps), _p(dwkl_dim),
                                              _p(lse_joint), _p(lse_dim), _stream()), what)
    return comps, dwkl_dim, lse_joint, lse_dim


def latent_decomposition_backward(z: torch.Tensor, mean: torch.Tensor, pre_var: torch.Tensor, lse_joint: torch.Tensor,
                                  lse_dim: torch.Tensor, coef: torch.Tensor):
    """The gradient of sum_{k,i} coef[k, i, :] . (mi, tc, dwkl)[k, i] with z, mean and pre_var held independent; ``lse_joint``
    / ``lse_dim``: ``latent_decomposition``'s of the same inputs, ``coef`` fp32 [K, B, 3] -> (dz [K, B, L], dmean [B, L],
    dpre_var [B, L]) (csrc/latent_decomp.hip)"""
    what = "latent_decomposition_backward"
    K, B, L = _decomp_args(what, z, mean, pre_var)
    _fp32(what, coef=coef)
    if coef.shape != (K, B, 3):
        raise ValueError("%s: coef %s for z %s (fp32 [K, B, 3])" % (what, tuple(coef.shape), (K, B, L)))
    for name, t, shape in (("lse_joint", lse_joint, (K, B)), ("lse_dim", lse_dim, (K, B, L))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.shape != shape or not t.is_contiguous():
            raise ValueError("%s: %s must be the forward's contiguous fp64 %s tensor" % (what, name, list(shape)))
    _need_gpu(z, mean, pre_var, lse_joint, lse_dim, coef)
    z, mean, pre_var, coef = z.contiguous(), mean.contiguous(), pre_var.contiguous(), coef.contiguous()
    dz, dmean, dpv = torch.empty_like(z), torch.empty_like(mean), torch.empty_like(pre_var)
    _lib.check(_lib.load().ggpm_latent_decomp_backward(_p(z), _p(mean), _p(pre_var), _p(lse_joint), _p(lse_dim), _p(coef), K, B, L,
                                                       _p(dz), _p(dmean), _p(dpv), _stream()), what)
    return dz, dmean, dpv


def latent_decomp_accumulate(comps: torch.Tensor, dwkl_dim: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """Adds the count K B and the sums over the draws of comps [K, B, 3] and of every column of dwkl_dim [K, B, L] to ``acc``,
    a contiguous fp64 [4 + L] device tensor the caller zeroed once -> acc (csrc/latent_decomp.hip)"""
    what = "latent_decomp_accumulate"
    _fp32(what, comps=comps, dwkl_dim=dwkl_dim)
    if dwkl_dim.dim() != 3 or dwkl_dim.numel() == 0 or comps.shape != tuple(dwkl_dim.shape[:2]) + (3,):
        raise ValueError("%s: comps %s / dwkl_dim %s must be [K, B, 3] and [K, B, L]" % (what, tuple(comps.shape), tuple(dwkl_dim.shape)))
    K, B, L = dwkl_dim.shape
    if K > LIKELIHOOD_MAX_K or B > LATENT_DECOMP_MAX_B or L > FREE_BITS_MAX_L or K * B * L >= 1 << 31:
        raise ValueError("%s: %d samples of %d molecules and %d latent columns are past the limits" % (what, K, B, L))
    if not isinstance(acc, torch.Tensor) or acc.shape != (LATENT_DECOMP_ROWS + L,) or acc.dtype != torch.float64 or \
            not acc.is_contiguous():
        raise ValueError("%s: acc must be a contiguous fp64 [%d] tensor" % (what, LATENT_DECOMP_ROWS + L))
    _need_gpu(comps, dwkl_dim, acc)
    comps, dwkl_dim = comps.contiguous(), dwkl_dim.contiguous()
    _lib.check(_lib.load().ggpm_latent_decomp_accumulate(_p(comps), _p(dwkl_dim), K, B, L, _p(acc), _stream()), what)
    return acc


MIXTURE_MAX_C = 4096            # include/ggpm_hip.h GGPM_MIXTURE_MAX_C


def _mixture_args(what: str, logits: torch.Tensor, means: torch.Tensor, log_vars: torch.Tensor, z: Optional[torch.Tensor] = None):
    """the checks the entries of the mixture prior share (no device needed for the ValueErrors) -> C, L and, with z, R"""
    _fp32(what, logits=logits, means=means, log_vars=log_vars, z=z)
    if means.dim() != 2 or means.numel() == 0 or log_vars.shape != means.shape or logits.shape != means.shape[:1]:
        raise ValueError("%s: logits %s / means %s / log_vars %s must be [C], [C, L] and [C, L]"
                         % (what, tuple(logits.shape), tuple(means.shape), tuple(log_vars.shape)))
    C, L = means.shape
    if C > MIXTURE_MAX_C or L > FREE_BITS_MAX_L:
        raise ValueError("%s: %d components over %d latent columns (at most %d and %d)" % (what, C, L, MIXTURE_MAX_C, FREE_BITS_MAX_L))
    if z is None:
        return C, L
    if z.dim() != 2 or z.shape[0] == 0 or z.shape[1] != L:
        raise ValueError("%s: z %s must be [R, %d]" % (what, tuple(z.shape), L))
    R = z.shape[0]
    if R * L >= 1 << 31 or R * C >= 1 << 31:
        raise ValueError("%s: %d rows of %d columns and %d components (fewer than 2^31 elements each way)" % (what, R, L, C))
    return C, L, R


def mixture_logp(z: torch.Tensor, logits: torch.Tensor, means: torch.Tensor, log_vars: torch.Tensor, want_resp: bool = False,
                 want_stash: bool = True):
    """z [R, L], the mixture's logits [C], means and log_vars [C, L] -> (logp fp32 [R]: the log-density of every row, ratio
    fp32 [R]: logp minus the standard normal's log-density, resp fp32 [R, C] or None: the responsibilities, comp_stash fp64
    [R, C] and logp_stash fp64 [R] or None: what the backward reads) (csrc/latent_prior.hip)"""
    what = "mixture_logp"
    C, L, R = _mixture_args(what, logits, means, log_vars, z)
    _need_gpu(z, logits, means, log_vars)
    z, logits, means, log_vars = z.contiguous(), logits.contiguous(), means.contiguous(), log_vars.contiguous()
    dev = z.device
    logp, ratio = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
    resp = torch.empty(R, C, dtype=torch.float32, device=dev) if want_resp else None
    comp_stash = torch.empty(R, C, dtype=torch.float64, device=dev) if want_stash else None
    logp_stash = torch.empty(R, dtype=torch.float64, device=dev) if want_stash else None
    _lib.check(_lib.load().ggpm_mixture_logp(_p(z), _p(logits), _p(means), _p(log_vars), R, C, L, _p(logp), _p(ratio), _p(resp),
                                             _p(comp_stash), _p(logp_stash), _stream()), what)
    return logp, ratio, resp, comp_stash, logp_stash


def mixture_logp_backward(z: torch.Tensor, logits: torch.Tensor, means: torch.Tensor, log_vars: torch.Tensor,
                          comp_stash: torch.Tensor, logp_stash: torch.Tensor, g: torch.Tensor, on_logp: bool,
                          want_dz: bool = True, want_params: bool = True):
    """The gradient of sum_r g[r] ratio[r] (``on_logp``: of sum_r g[r] logp[r]) of ``mixture_logp``; the stashes are the
    forward's, of the same inputs, ``g`` fp32 [R] -> (dz [R, L] or None, dmeans [C, L], dlog_vars [C, L], dlogits [C] or three
    None): one launch for dz, one for the parameters' three (csrc/latent_prior.hip)"""
    what = "mixture_logp_backward"
    C, L, R = _mixture_args(what, logits, means, log_vars, z)
    _fp32(what, g=g)
    if g.shape != (R,):
        raise ValueError("%s: g %s for %d rows (fp32 [R])" % (what, tuple(g.shape), R))
    for name, t, shape in (("comp_stash", comp_stash, (R, C)), ("logp_stash", logp_stash, (R,))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.shape != shape or not t.is_contiguous():
            raise ValueError("%s: %s must be the forward's contiguous fp64 %s tensor" % (what, name, list(shape)))
    if not want_dz and not want_params:
        raise ValueError("%s: neither dz nor the parameters' gradients are asked for" % what)
    _need_gpu(z, logits, means, log_vars, comp_stash, logp_stash, g)
    z, logits, means, log_vars, g = z.contiguous(), logits.contiguous(), means.contiguous(), log_vars.contiguous(), g.contiguous()
    dz = torch.empty_like(z) if want_dz else None
    dm, ds, da = (torch.empty_like(means), torch.empty_like(log_vars), torch.empty_like(logits)) if want_params else (None,) * 3
    _lib.check(_lib.load().ggpm_mixture_logp_backward(_p(z), _p(logits), _p(means), _p(log_vars), _p(comp_stash), _p(logp_stash),
                                                      _p(g), int(bool(on_logp)), R, C, L, _p(dz), _p(dm), _p(ds), _p(da),
                                                      _stream()), what)
    return dz, dm, ds, da


def sample_mixture(logits: torch.Tensor, means: torch.Tensor, log_vars: torch.Tensor, rows: int, seed_lo: int, seed_hi: int,
                   ids=None, want_components: bool = False):
    """[rows, L] draws from the mixture on the seeded stream (csrc/latent_prior.hip): row r, keyed by ``ids[r]`` (default
    ``arange``), takes its component from one uniform of site PRIOR_COMP and then m + exp(s / 2) n with ``sample_normal``'s
    n for the same seed and id -> (out, the int32 [rows] components or None)"""
    what = "sample_mixture"
    C, L = _mixture_args(what, logits, means, log_vars)
    rows = int(rows)
    if rows < 1 or rows * L >= 1 << 31 or rows * C >= 1 << 31:
        raise ValueError("%s: %d rows of %d columns and %d components (at least one row, fewer than 2^31 elements each way)"
                         % (what, rows, L, C))
    ids = torch.arange(rows, dtype=torch.int32) if ids is None else torch.as_tensor(ids).to(torch.int64).bitwise_and(
        0xFFFFFFFF).to(torch.int32)
    if ids.shape != (rows,):
        raise ValueError("%s: %d ids for %d rows" % (what, ids.numel(), rows))
    _need_gpu(logits, means, log_vars)
    logits, means, log_vars = logits.contiguous(), means.contiguous(), log_vars.contiguous()
    dev = means.device
    out = torch.empty(rows, L, dtype=torch.float32, device=dev)
    comp = torch.empty(rows, dtype=torch.int32, device=dev) if want_components else None
    ids = ids.to(dev)
    _lib.check(_lib.load().ggpm_sample_mixture(_p(logits), _p(means), _p(log_vars), C, _p(out), rows, L, L, _p(ids),
                                               seed_lo & 0xFFFFFFFF, seed_hi & 0xFFFFFFFF, _p(comp), _stream()), what)
    return out, comp


def padded_hidden(H: int) -> int:
    return (H + 15) // 16 * 16


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D tensor expected"
    return t.stride(0)


def _empty_same_layout(x: torch.Tensor) -> torch.Tensor:
    """An uninitialised [rows, cols] tensor with x's leading dimension.  (``torch.empty_like`` of a column slice of a
    padded buffer -- e.g. the [rows, H + 20] view of a [rows, ld] message-input buffer when H + 20 is not a multiple
    of 4 -- returns a DENSE tensor, whose leading dimension is not x's.)"""
    return torch.empty(x.shape[0], _ld(x), dtype=x.dtype, device=x.device)[:, :x.shape[1]]


# ----------------------------------------------------------------------------- graph layout
class CSR:
    """Device CSR (int32 rowptr[rows+1], col[cap]) plus its lazily built transpose."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, rows: int, ncols: int):
        self.rowptr, self.col, self.rows, self.ncols = rowptr, col, rows, ncols
        self._T: Optional["CSR"] = None
        self._back = None           # on a transpose: weak reference to the CSR it was built from (a strong one would make the
        self._T_event = None        # pair a reference cycle, and its device tensors would wait for Python's collector)
        self._keep = None

    def _build_T(self) -> "CSR":
        lib = _lib.load()
        dev = self.col.device
        rowptrT = torch.empty(self.ncols + 1, dtype=torch.int32, device=dev)
        colT = torch.empty(max(self.col.numel(), 1), dtype=torch.int32, device=dev)
        cursor = torch.empty(self.ncols, dtype=torch.int32, device=dev)
        _lib.check(lib.ggpm_csr_transpose(_p(self.rowptr), _p(self.col), self.rows, self.ncols, _p(rowptrT),
                                          _p(colT), _p(cursor), _stream()), "csr_transpose")
        t = CSR(rowptrT, colT, self.ncols, self.rows)
        t._back = weakref.ref(self)
        t._keep = cursor
        return t

    @property
    def T(self) -> "CSR":
        if self._T is None:
            back = self._back() if self._back is not None else None
            if back is not None:
                return back
            self._T = self._build_T()
        ev = self._T_event
        if ev is not None:          # built ahead of time on the second stream: order this stream behind it once
            torch.cuda.current_stream().wait_event(ev)
            self._T_event = None
        return self._T


def prefetch_transposes(csrs: Sequence["CSR"]) -> None:
    """Build the transposes the BACKWARD will need on the second stream while the forward runs (each is a
    single-workgroup integer kernel of ~10 us that would otherwise sit on the backward's critical path)."""
    todo = [c for c in csrs if c is not None and c._T is None and (c._back is None or c._back() is None)]
    if not todo or not side_stream_enabled():
        return
    main = torch.cuda.current_stream()
    side = _side_stream(todo[0].col.device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        for c in todo:
            c._T = c._build_T()
            for t in (c.rowptr, c.col):
                t.record_stream(side)
        ev = torch.cuda.Event()
        ev.record(side)
    for c in todo:
        for t in (c._T.rowptr, c._T.col, c._T._keep):
            t.record_stream(main)
        c._T_event = ev


class _StagingRing:
    """Pinned staging for host -> device uploads of numpy tables (decode schedules, atom plans): ``pin_memory()`` on a
    fresh tensor is a cudaHostAlloc of several milliseconds per call -- more than the copy -- so the bytes go through a
    small ring of pinned buffers that are allocated once and grow on demand."""

    def __init__(self, slots: int = 8):      # (three uploads per batch in the vae_train.py call shape: a slot is reused 2-3 batches later)
        self.slots, self.bufs, self.events, self.i = slots, [None] * slots, [None] * slots, 0

    def upload(self, a, device) -> torch.Tensor:
        import numpy as np
        a = np.ascontiguousarray(a)
        out = torch.empty(a.shape, dtype=torch.from_numpy(a[:0].reshape(0)).dtype, device=device)
        if a.size == 0:
            return out
        if torch.device(device).type != "cuda":
            out.copy_(torch.from_numpy(a))
            return out
        k = self.i
        self.i = (self.i + 1) % self.slots
        if self.events[k] is not None:
            self.events[k].synchronize()          # slot reuse: its previous copy must have left the buffer
        if self.bufs[k] is None or self.bufs[k].numel() < a.nbytes:
            self.bufs[k] = torch.empty(max(a.nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        stage = self.bufs[k][:a.nbytes]
        # a plain memcpy into the pinned buffer: torch's CPU copy_ fans a 1 MB copy out over every visible core, whose
        # OpenMP team then spins beside the training thread (on a box with a 16-CPU quota the whole process gets
        # throttled: 35 instead of 12 ms per step when the decode schedule is uploaded inside the step)
        np.copyto(stage.numpy(), a.reshape(-1).view(np.uint8))
        out.view(-1).view(torch.uint8).copy_(stage, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        return out


_STAGING = _StagingRing()


def upload(a, device) -> torch.Tensor:
    """numpy array -> device tensor of the same dtype and shape through the pinned staging ring (asynchronous)."""
    return _STAGING.upload(a, device)


_MEMO_ON = None        # None: _dev.INDEX_MEMO, read at call time; True / False: forced (bench.py's "index structures rebuilt" leg)


def _memo_get(t: torch.Tensor, slot: str, key):
    """Index structures derived from an index tensor are remembered ON that tensor object, keyed by its in-place
    version counter: a batch whose tables stay resident -- a DecodeSchedule on the device, the encoder's graph
    tensors -- pays for their CSRs and transposes once, not once per step."""
    if not (_dev.INDEX_MEMO if _MEMO_ON is None else _MEMO_ON):
        return None
    m = getattr(t, slot, None)
    # `_version` counts in-place writes: a resident index tensor that is refilled (``t.copy_(next_batch)``) must not
    # be served the structures of its old contents
    return m[2] if m is not None and m[0] == key and m[1] == version_of(t) else None


def _memo_put(t: torch.Tensor, slot: str, key, value):
    if torch.is_inference_mode_enabled() and not t.is_inference():
        return value        # (structures made under inference_mode must not outlive it on a tensor that training reuses)
    try:
        setattr(t, slot, (key, version_of(t), value))
    except AttributeError:
        pass
    return value


def csr_from_padded(padded: torch.Tensor, ncols: int) -> CSR:
    """agraph/bgraph/cgraph (int64 [rows, width], 0 = no entry) -> CSR over the real entries."""
    _need_gpu(padded)
    assert padded.dtype == torch.int64 and padded.dim() == 2
    hit = _memo_get(padded, "_ggpm_csr", ncols)
    if hit is not None:
        return hit
    owner = padded
    padded = padded.contiguous()
    rows, width = padded.shape
    rowptr = torch.empty(rows + 1, dtype=torch.int32, device=padded.device)
    col = torch.empty(max(rows * width, 1), dtype=torch.int32, device=padded.device)
    _lib.check(_lib.load().ggpm_padded_to_csr(_p(padded), rows, width, _p(rowptr), _p(col), _stream()),
               "padded_to_csr")
    return _memo_put(owner, "_ggpm_csr", ncols, CSR(rowptr, col, rows, ncols))


def csr_from_index(idx: torch.Tensor, ncols: int) -> CSR:
    """One entry per row (col = idx[row]); its transpose lists, per id, the rows that use it."""
    hit = _memo_get(idx, "_ggpm_csr_index", ncols)
    if hit is not None:
        return hit
    rows = idx.numel()
    rowptr = torch.arange(rows + 1, dtype=torch.int32, device=idx.device)
    # (the remembered CSR holds an alias of `idx`, not the object the memo hangs on: no reference cycle)
    return _memo_put(idx, "_ggpm_csr_index", ncols, CSR(rowptr, idx.detach(), rows, ncols))


def extract_column(mat: torch.Tensor, column: int) -> torch.Tensor:
    _need_gpu(mat)
    assert mat.dtype == torch.int64
    if mat.dim() == 1:
        mat = mat.unsqueeze(1)
    mat = mat.contiguous()
    out = torch.empty(mat.shape[0], dtype=torch.int32, device=mat.device)
    _lib.check(_lib.load().ggpm_extract_column(_p(mat), mat.shape[0], mat.shape[1], column, _p(out), _stream()),
               "extract_column")
    return out


# ----------------------------------------------------------------------------- raw launches
def gemm(ta: int, tb: int, M: int, N: int, K: int, A: torch.Tensor, lda: int, B: torch.Tensor, ldb: int,
         C: torch.Tensor, ldc: int, n_pad: int, bias: Optional[torch.Tensor] = None, accumulate: bool = False,
         act: int = ACT_NONE, zero_row0: bool = False, splitk: bool = False) -> None:
    lib = _lib.load()
    ws, wsb = None, 0
    if splitk:
        wsb = int(lib.ggpm_gemm_workspace_bytes(M, N, K))
        if wsb:
            ws = torch.empty(wsb // 4, dtype=torch.float32, device=C.device)
    _lib.check(lib.ggpm_gemm(ta, tb, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, n_pad, _p(bias),
                             int(accumulate), act, int(zero_row0), _p(ws), wsb, _stream()), "gemm")


class WgradItem(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_wgrad_item"""
    _fields_ = [("dpre", ctypes.c_void_p), ("ld_dpre", ctypes.c_int), ("x", ctypes.c_void_p), ("ld_x", ctypes.c_int),
                ("dW", ctypes.c_void_p), ("ld_dw", ctypes.c_int), ("db", ctypes.c_void_p), ("M", ctypes.c_int), ("N", ctypes.c_int),
                ("K", ctypes.c_int)]


class GemmProblem(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_gemm_problem"""
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int), ("B", ctypes.c_void_p), ("ldb", ctypes.c_int),
                ("C", ctypes.c_void_p), ("ldc", ctypes.c_int), ("n_pad", ctypes.c_int), ("bias", ctypes.c_void_p),
                ("accumulate", ctypes.c_int), ("act", ctypes.c_int), ("zero_row0", ctypes.c_int)]


class PairProblem(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_pair_problem"""
    _fields_ = [("hi", ctypes.c_void_p), ("lo", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p),
                ("ldc", ctypes.c_int)]


_I4 = ctypes.c_int * 4
GEMM_ENTRIES = ("gemm", "grouped", "grouped_splitk", "grouped_masked", "ksegments", "tall_grouped", "pair_grouped", "tn_bf16")
GEMM_KERNELS = ("none", "gemm_kernel", "gemm_kernel_segs", "gemm_kernel_group", "gemm_kernel_v2", "gemm_group_v2",
                "gemm_small_v3", "gemm_tn_tall", "gemm_tn_tall_bf16<false>", "gemm_tn_tall_bf16<true>", "gemm_tn_tall_split",
                "sequence")
GEMM_REDUCES = ("none", "splitk_reduce", "splitk_reduce_group", "tall_reduce")


class GemmCall(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_gemm_call -- what the GEMM dispatchers look at"""
    _fields_ = [("entry", ctypes.c_int), ("trans_a", ctypes.c_int), ("trans_b", ctypes.c_int), ("M", ctypes.c_int),
                ("N", ctypes.c_int), ("count", ctypes.c_int), ("K", _I4), ("lda", _I4), ("ldb", _I4), ("ldc", _I4),
                ("n_pad", _I4), ("base_a", _I4), ("base_b", _I4), ("base_lo", _I4), ("has_ws", ctypes.c_int),
                ("mode", ctypes.c_int), ("ws_bytes", ctypes.c_size_t)]


class GemmForm(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_gemm_form -- the kernel, reduce, split and grid a GEMM call takes"""
    _fields_ = [("kernel", ctypes.c_int), ("vec_a", ctypes.c_int), ("vec_b", ctypes.c_int), ("reduce", ctypes.c_int),
                ("splits", ctypes.c_int), ("k_chunk", _I4), ("grid", ctypes.c_int * 3), ("rc", ctypes.c_int),
                ("lds_bytes", ctypes.c_size_t), ("ws_used", ctypes.c_size_t)]


def gemm_form(entry: str, ta: int, tb: int, M: int, N: int, K, lda, ldb, ldc, n_pad, base_a=0, base_b=0, base_lo=0,
              count: int = 1, ws_bytes: Optional[int] = None, mode: int = 0) -> GemmForm:
    """ggpm_gemm_form_query: the form the GEMM entry point ``entry`` (GEMM_ENTRIES) takes for this call -> GemmForm, whose
    ``rc`` is what the call itself would return.  K, the leading dimensions, n_pad and the low address bits are per member
    (an int stands for every member); ``ws_bytes`` None: no workspace passed.  Host only: needs no GPU."""
    def four(v):
        v = list(v) if isinstance(v, (list, tuple)) else [v] * 4
        return _I4(*(v + [0] * (4 - len(v))))
    call = GemmCall(GEMM_ENTRIES.index(entry), ta, tb, M, N, count, four(K), four(lda), four(ldb), four(ldc), four(n_pad),
                    four(base_a), four(base_b), four(base_lo), int(ws_bytes is not None), mode, ws_bytes or 0)
    out = GemmForm()
    _lib.check(_lib.load().ggpm_gemm_form_query(ctypes.byref(call), ctypes.byref(out)), "gemm_form_query")
    return out


class LevelOpts(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_level_opts -- the options of ONE level call (None: all defaults)"""
    _fields_ = [("gate_dtype", ctypes.c_int), ("prefer_narrow", ctypes.c_int), ("weights_packed", ctypes.c_int),
                ("defer_stash", ctypes.c_void_p * 4), ("gather_h", ctypes.c_void_p), ("gather_c", ctypes.c_void_p),
                ("gather_idx", ctypes.c_void_p), ("scatter_h", ctypes.c_void_p), ("scatter_c", ctypes.c_void_p),
                ("scatter_idx", ctypes.c_void_p), ("skip_x_sums", ctypes.c_int), ("run_depth", ctypes.c_int),
                ("lo", ctypes.c_int), ("skip_bias_u", ctypes.c_int), ("skip_sparse_wgrads", ctypes.c_int),
                ("h_out", ctypes.c_void_p), ("c_out", ctypes.c_void_p), ("fixed_slot", ctypes.c_int),
                ("q_part", ctypes.c_void_p), ("q_part_bytes", ctypes.c_size_t)]


class LevelForm(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_level_form -- the launch geometry, gate mode and LDS sizes a level call takes"""
    _fields_ = [("Hp", ctypes.c_int), ("tiles", ctypes.c_int), ("tg", ctypes.c_int), ("groups", ctypes.c_int),
                ("rt2", ctypes.c_int), ("gate_mode", ctypes.c_int), ("st16", ctypes.c_int), ("fuse_fwd", ctypes.c_int),
                ("fuse_bwd", ctypes.c_int), ("lds_fwd_a", ctypes.c_size_t), ("lds_fwd_b", ctypes.c_size_t),
                ("lds_bwd_a", ctypes.c_size_t), ("lds_bwd_b", ctypes.c_size_t)]


def level_form(lstm: bool, E1: int, H: int, sparse: bool = False, training: bool = True, opts: Optional[LevelOpts] = None):
    """ggpm_level_form_query: the form a GRU / LSTM level call of ``E1`` rows and hidden size ``H`` takes -> LevelForm, or
    None for a shape the level entry points refuse (GGPM_ERR_UNSUPPORTED).  Host only: needs no GPU."""
    out = LevelForm()
    rc = _lib.load().ggpm_level_form_query(int(lstm), E1, H, int(sparse), int(training),
                                           None if opts is None else ctypes.byref(opts), ctypes.byref(out))
    if rc == _lib.GGPM_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "level_form_query")
    return out


_GATE_OPTS = {dt: LevelOpts(gate_dtype=dt) for dt in (1, 2, 3)}


def _gate_opts(gate_dtype: int):
    """The options of a dense level call on gate-product dtype ``gate_dtype`` (0: None, the defaults)."""
    o = _GATE_OPTS.get(gate_dtype)
    return None if o is None else ctypes.byref(o)


def gemm_grouped(ta: int, tb: int, M: int, N: int, K: int, problems, splitk: bool = False) -> None:
    """problems: list of dicts(A, lda, B, ldb, C, ldc, n_pad, bias=None, accumulate=False, act=ACT_NONE, zero_row0=False);
    up to four independent products of one shape in one launch.  ``splitk``: the K range in chunks where the group has few
    output tiles and a long K (ggpm_gemm_grouped_splitk: weight gradients over all rows of a level)."""
    lib = _lib.load()
    arr = _lib.array_type(GemmProblem, len(problems))()
    for i, q in enumerate(problems):
        arr[i] = GemmProblem(_p(q["A"]), q["lda"], _p(q["B"]), q["ldb"], _p(q["C"]), q["ldc"], q["n_pad"],
                             _p(q.get("bias")), int(q.get("accumulate", False)), q.get("act", ACT_NONE),
                             int(q.get("zero_row0", False)))
    wsb = int(lib.ggpm_gemm_grouped_splitk_workspace_bytes(M, N, K, len(problems))) if splitk else 0
    if wsb:
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=problems[0]["C"].device)
        _lib.check(lib.ggpm_gemm_grouped_splitk(ta, tb, M, N, K, len(problems), ctypes.addressof(arr), _p(ws), wsb,
                                                _stream()), "gemm_grouped_splitk")
        return
    _lib.check(lib.ggpm_gemm_grouped(ta, tb, M, N, K, len(problems), ctypes.addressof(arr), _stream()),
               "gemm_grouped")


def head_accuracies(cls_pred, cls_lab, icls_pred, icls_lab, topo, topo_lab, assm) -> torch.Tensor:
    """-> [4] float tensor {motif-class, attachment-class, topology, attachment accuracy} (ggpm_head_accuracies: one launch).
    ``cls_pred`` / ``icls_pred``: int32 arg-max per row; ``topo``: 1-D scores (any stride); ``assm``: [P, C] scores or None."""
    _need_gpu(topo, cls_pred)
    out = torch.empty(4, dtype=torch.float32, device=topo.device)
    lab64 = int(cls_lab.dtype == torch.int64)
    labs = [t if t.is_contiguous() else t.contiguous() for t in (cls_lab, icls_lab, topo_lab)]
    preds = [t if (t.dtype == torch.int32 and t.is_contiguous()) else t.to(torch.int32).contiguous() for t in (cls_pred, icls_pred)]
    n_topo = topo.numel()
    ld_topo = topo.stride(0) if n_topo > 1 else 1
    P_, C_, ld_assm = (assm.shape[0], assm.shape[1], assm.stride(0)) if assm is not None else (0, 1, 1)
    _lib.check(_lib.load().ggpm_head_accuracies(_p(preds[0]), _p(labs[0]), _p(preds[1]), _p(labs[1]), preds[0].numel(), _p(topo),
                                                ld_topo, _p(labs[2]), n_topo, _p(assm), ld_assm, P_, C_, lab64, _p(out),
                                                _stream()), "head_accuracies")
    return out


def gemm_ksegments(tb: int, M: int, N: int, As, ldas, Bs, ldbs, Ks, C: torch.Tensor, ldc: int, n_pad: int,
                   bias: Optional[torch.Tensor] = None, accumulate: bool = False, act: int = ACT_NONE,
                   zero_row0: bool = False) -> None:
    """C = act(sum_s A_s B_s' + bias (+ C)) in one launch (up to four K segments)."""
    n = len(As)
    vp, ci = _lib.array_type(ctypes.c_void_p, n), _lib.array_type(ctypes.c_int, n)
    pa, pb = vp(*[_p(a) for a in As]), vp(*[_p(b) for b in Bs])
    la, lb, kk = ci(*ldas), ci(*ldbs), ci(*Ks)
    cast = ctypes.addressof          # (ctypes.cast would leave each array in a reference cycle with itself)
    _lib.check(_lib.load().ggpm_gemm_ksegments(tb, M, N, n, cast(pa), cast(la), cast(pb), cast(lb), cast(kk), _p(C), ldc,
                                               n_pad, _p(bias), int(accumulate), act, int(zero_row0), _stream()),
               "gemm_ksegments")


def colsum(A: torch.Tensor, M: int, N: int) -> torch.Tensor:
    out = torch.empty(N, dtype=torch.float32, device=A.device)
    ws = torch.empty(256 * N, dtype=torch.float32, device=A.device)
    _lib.check(_lib.load().ggpm_colsum(_p(A), _ld(A), M, N, _p(out), _p(ws), _stream()), "colsum")
    return out


def _segment_sum_raw(src: torch.Tensor, csr: CSR, width: int, out: torch.Tensor) -> None:
    """out[:, :width] = segmented sums; the kernel also zeroes the pad columns [width, out.shape[1])."""
    _lib.check(_lib.load().ggpm_segment_sum(_p(src), _ld(src), _p(csr.rowptr), _p(csr.col), csr.rows, width,
                                            _p(out), _ld(out), 0, out.shape[1], _stream()), "segment_sum")


# ----------------------------------------------------------------------------- autograd functions
class _Linear(torch.autograd.Function):
    """y[:, :N] = act( sum_i x_i[:, :K_i] W[:, off_i:off_i+K_i]^T + b ), pad columns of y zero."""

    @staticmethod
    def forward(ctx, weight, bias, act, zero_row0, ld_out, Ks, *xs):
        _need_gpu(weight, *xs)
        N = weight.shape[0]
        M = xs[0].shape[0]
        assert sum(Ks) == weight.shape[1] and weight.stride(1) == 1
        y = torch.empty(M, ld_out, dtype=torch.float32, device=weight.device)
        if 1 < len(xs) <= 4:        # the inputs are K segments of ONE product: no cat, no read-modify-write of y
            offs = [sum(Ks[:i]) for i in range(len(Ks))]
            gemm_ksegments(1, M, N, list(xs), [_ld(x) for x in xs], [weight[:, o:] for o in offs],
                           [weight.stride(0)] * len(xs), list(Ks), y, ld_out, ld_out, bias=bias, act=act,
                           zero_row0=zero_row0)
        else:
            off = 0
            last = len(xs) - 1
            for i, (x, K) in enumerate(zip(xs, Ks)):
                wv = weight[:, off:]
                gemm(0, 1, M, N, K, x, _ld(x), wv, weight.stride(0), y, ld_out, ld_out,
                     bias=bias if i == 0 else None, accumulate=i > 0, act=act if i == last else ACT_NONE,
                     zero_row0=zero_row0 and i == last)
                off += K
        ctx.save_for_backward(weight, y, *xs)
        ctx.meta = (act, zero_row0, Ks, bias is not None)
        ctx.weight_ref, ctx.bias_ref = weight, bias       # the Parameter objects themselves (their .grad is assigned)
        return y

    @staticmethod
    def backward(ctx, dy):
        weight, y, *xs = ctx.saved_tensors
        act, zero_row0, Ks, has_bias = ctx.meta
        N = weight.shape[0]
        M = y.shape[0]
        dy = dy.contiguous() if dy.stride(1) != 1 else dy
        lib = _lib.load()
        if act != ACT_NONE or zero_row0:
            dpre = torch.empty_like(y)
            assert _ld(dy) == _ld(y)
            _lib.check(lib.ggpm_act_backward(_p(dy), _p(y), M, N, _ld(y), act, int(zero_row0), _p(dpre), _stream()),
                       "act_backward")
        else:
            dpre = dy
        dxs: List[Optional[torch.Tensor]] = []
        off = 0
        for i, (x, K) in enumerate(zip(xs, Ks)):     # input gradients are needed upstream right away: main stream
            if ctx.needs_input_grad[6 + i]:
                dx = torch.empty_like(x)
                gemm(0, 0, M, K, N, dpre, _ld(dpre), weight[:, off:], weight.stride(0), dx, _ld(dx), x.shape[1])
                dxs.append(dx)
            else:
                dxs.append(None)
            off += K

        def param_grads():
            dW_ = torch.empty_like(weight) if ctx.needs_input_grad[0] else None
            o = 0
            for x, K in zip(xs, Ks):
                if dW_ is not None:
                    gemm(1, 0, N, K, M, dpre, _ld(dpre), x, _ld(x), dW_[:, o:], dW_.stride(0), K, splitk=True)
                o += K
            db_ = colsum(dpre, M, N) if (has_bias and ctx.needs_input_grad[1]) else None
            return dW_, db_

        wref, bias = ctx.weight_ref, ctx.bias_ref
        leaf = (ctx.needs_input_grad[0] and (bias is None or ctx.needs_input_grad[1]) and can_publish(wref, bias))
        if leaf and defer_wgrads_enabled():       # one contraction per parameter at the end of the pass (see _DeferredGrads)
            _defer_linear(wref, bias, dpre, list(xs), Ks)
            return (None, None, None, None, None, None, *dxs)
        use_side = side_stream_enabled() and leaf
        if use_side:      # weight / bias gradients: second stream, straight into param.grad (as the level functions do)
            publish_aside(weight.device, (dpre, *xs), (wref, bias), param_grads)
            return (None, None, None, None, None, None, *dxs)
        dW, db = param_grads()
        return (dW, db, None, None, None, None, *dxs)


def linear(xs: Sequence[torch.Tensor], Ks: Sequence[int], weight: torch.Tensor, bias: Optional[torch.Tensor],
           act: int = ACT_NONE, zero_row0: bool = False, ld_out: Optional[int] = None) -> torch.Tensor:
    N = weight.shape[0]
    if ld_out is None:
        ld_out = padded_hidden(N)
    return _Linear.apply(weight, bias, act, zero_row0, ld_out, tuple(Ks), *xs)


class _SegmentSum(torch.autograd.Function):
    """out[r] = sum_{j in csr row r} src[col[j]]  (index_select_ND(...).sum(1) over real entries)."""

    @staticmethod
    def forward(ctx, src, csr, width):
        _need_gpu(src)
        out = torch.empty(csr.rows, _ld(src), dtype=torch.float32, device=src.device)
        _segment_sum_raw(src, csr, width, out)
        ctx.csr, ctx.width, ctx.src_rows, ctx.src_cols = csr, width, src.shape[0], src.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous() if dout.stride(1) != 1 else dout
        csrT = ctx.csr.T
        assert csrT.rows == ctx.src_rows
        dsrc = torch.empty(ctx.src_rows, _ld(dout), dtype=torch.float32, device=dout.device)
        _segment_sum_raw(dout, csrT, ctx.width, dsrc)
        return dsrc[:, :ctx.src_cols], None, None     # src may have been a [rows, H] view of a padded buffer


def segment_sum(src: torch.Tensor, csr: CSR, width: int) -> torch.Tensor:
    return _SegmentSum.apply(src, csr, width)


class _GatherRows(torch.autograd.Function):
    """out[r, :width] = table[idx[r], :width] (nn.Embedding / index_select); backward through idx^T."""

    @staticmethod
    def forward(ctx, table, idx, idx_csr, width, ld_out):
        _need_gpu(table, idx)
        rows = idx.numel()
        out = torch.empty(rows, ld_out, dtype=torch.float32, device=table.device)
        _lib.check(_lib.load().ggpm_gather_rows(_p(table), _ld(table), _p(idx), rows, width, _p(out), ld_out, 0,
                                                ld_out, _stream()), "gather_rows")
        ctx.idx_csr, ctx.width, ctx.tshape, ctx.tld = idx_csr, width, table.shape, _ld(table)
        ctx.table_ref, ctx.idx = table, idx
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous() if dout.stride(1) != 1 else dout
        if ctx.needs_input_grad[0] and can_publish(ctx.table_ref) and defer_wgrads_enabled():
            _defer_gather(ctx.table_ref, ctx.width, dout, ctx.idx)      # one scatter over the rows of all visits at the end of the pass
            return None, None, None, None, None
        csrT = ctx.idx_csr.T
        dtable = torch.empty(ctx.tshape, dtype=torch.float32, device=dout.device)
        _segment_sum_raw(dout, csrT, ctx.width, dtable)
        return dtable, None, None, None, None


def gather_rows(table: torch.Tensor, idx: torch.Tensor, idx_csr: CSR, width: int, ld_out: int) -> torch.Tensor:
    return _GatherRows.apply(table, idx, idx_csr, width, ld_out)


class _TreeMessInput(torch.autograd.Function):
    """hmess = [hnode[src] | onehot(pos)]  (embed_inter/embed_tree, ggpm/encoder.py:103-106,114-116)."""

    @staticmethod
    def forward(ctx, hnode, src, src_csr, pos, H, n_pos, ld_out):
        _need_gpu(hnode, src, pos)
        lib = _lib.load()
        rows = src.numel()
        out = torch.empty(rows, ld_out, dtype=torch.float32, device=hnode.device)
        _lib.check(lib.ggpm_gather_rows(_p(hnode), _ld(hnode), _p(src), rows, H, _p(out), ld_out, 0, 0, _stream()),
                   "gather_rows")
        _lib.check(lib.ggpm_onehot(_p(pos), rows, n_pos, _p(out), ld_out, H, ld_out, _stream()), "onehot")
        ctx.src_csr, ctx.H, ctx.nshape = src_csr, H, hnode.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous() if dout.stride(1) != 1 else dout
        csrT = ctx.src_csr.T
        dh = torch.empty(ctx.nshape, dtype=torch.float32, device=dout.device)
        _segment_sum_raw(dout, csrT, ctx.H, dh)
        return dh, None, None, None, None, None, None


def tree_message_input(hnode, src, src_csr, pos, H, n_pos, ld_out):
    return _TreeMessInput.apply(hnode, src, src_csr, pos, H, n_pos, ld_out)


def embed_graph(fnode: torch.Tensor, fmess: torch.Tensor, atom_size: int, bond_types: int, max_pos: int
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One-hot atom-level inputs (constants: no gradient), ggpm/encoder.py:119-126."""
    _need_gpu(fnode, fmess)
    N1, E1 = fnode.shape[0], fmess.shape[0]
    ld_n = (atom_size + 3) // 4 * 4
    ld_m = (atom_size + bond_types + max_pos + 3) // 4 * 4
    hnode = torch.empty(N1, ld_n, dtype=torch.float32, device=fnode.device)
    hmess = torch.empty(E1, ld_m, dtype=torch.float32, device=fnode.device)
    _lib.check(_lib.load().ggpm_embed_graph(_p(fnode.contiguous()), N1, _p(fmess.contiguous()), E1, atom_size,
                                            bond_types, max_pos, _p(hnode), ld_n, _p(hmess), ld_m, _stream()),
               "embed_graph")
    return hnode, hmess


# ----------------------------------------------------------------------------- second stream for weight gradients
# The depth loops are latency bound (small dependent kernels); the weight-gradient GEMMs over the stashes are
# throughput bound and independent of the remaining backward.  With GGPM_SIDE_STREAM=1 (default) they run on
# a second HIP stream beside the next level's depth loop and accumulate straight into ``param.grad``; the main
# stream re-joins at the end of the backward pass (autograd engine callback), so after ``loss.backward()``
# returns every later main-stream consumer (clip_grad_norm_, all-reduce, optimizer) is ordered behind them.
# Contract: a parameter whose gradient is published this way must be consumed ONLY by the ops of this module inside the
# backward pass (true for every parameter of the encoder / decoder classes of this package, tied embeddings included:
# both users go through these ops).  A stock torch op on the same leaf would have autograd's AccumulateGrad add to
# ``.grad`` on the main stream while the second stream may still be writing it -- route such a use through
# GGPM_SIDE_STREAM=0, which keeps every gradient on the main stream and inside autograd.
_HELPER_STREAMS = {}        # (device index, kind in "second", "atom") -> every helper stream that writes gradients


def side_stream_enabled() -> bool:
    import os
    return os.environ.get("GGPM_SIDE_STREAM", "1") != "0"


def helper_stream(device, kind: str, priority: int = 0) -> torch.cuda.Stream:
    """The package's one stream of `kind` on `device`: "second" (weight gradients, index transposes) or "atom" (the
    decoder's atom level, decoder.start_atom_level).  Created on first use, with the priority of that first request
    (ROCm offers priorities 0 and -1 only: nothing below normal)."""
    assert kind in ("second", "atom"), kind
    key = (device.index if device.index is not None else torch.cuda.current_device(), kind)
    if key not in _HELPER_STREAMS:
        _HELPER_STREAMS[key] = torch.cuda.Stream(device=device, priority=priority)
    return _HELPER_STREAMS[key]


def _side_stream(device) -> torch.cuda.Stream:
    return helper_stream(device, "second")


def writer_streams(device) -> list:
    """Every helper stream of the package in use on `device` (parallel.FlatGradSync._join_writers orders its collective
    behind each of them)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    return [_HELPER_STREAMS[index, kind] for kind in ("second", "atom") if (index, kind) in _HELPER_STREAMS]


# A gradient tensor computed on a helper stream (second stream, atom-level stream) and then read on the main stream
# (optimizer, clipping, the flat-buffer pack) would ordinarily be marked with ``record_stream(main)``.  On ROCm every such
# mark costs an event record on that stream when the tensor is released -- ~4.7 us of queue time each, and the ~55
# gradients of a VAE step are released together right in front of the optimizer launch (0.25 ms of idle GPU, measured:
# tools/probe/free_stall_probe.py).  The mark is not needed here: a published gradient stays referenced by ``param.grad``
# until the optimizer side releases it, i.e. after everything that reads it has been ENQUEUED on the main stream, and every
# helper stream of this package waits for the main stream (``wait_stream(main)``) before the first allocation of its next use
# -- the block cannot be handed out again in front of its readers.  _dev.RECORD_GRADS restores the marks.


def hand_to(g: torch.Tensor, main: torch.cuda.Stream) -> None:
    if _dev.RECORD_GRADS:
        g.record_stream(main)


def second_backward(node: str) -> RuntimeError:
    """The error of a node whose first backward has released the state it saved (to free it early): a second backward
    through the same graph -- loss.backward(retain_graph=True), then backward again -- is not supported."""
    return RuntimeError("%s: a retained graph is not supported: backward through the same graph a second time "
                        "(retain_graph=True) finds the state released by the first backward; run the forward again" % node)


def _accumulate_grad(param: torch.Tensor, g: torch.Tensor, main: torch.cuda.Stream) -> None:
    """param.grad (+)= g on the CURRENT stream; `main` is the stream the gradient is consumed on (hand_to)."""
    hand_to(g, main)
    if param.grad is None:
        param.grad = g
    else:
        param.grad.add_(g)


def _join_later(main: torch.cuda.Stream, side: torch.cuda.Stream) -> None:
    torch.autograd.Variable._execution_engine.queue_callback(lambda: main.wait_stream(side))


def publish_aside(device, reads, params, grads_fn) -> None:
    """Form parameter gradients on the second stream and add them into ``.grad`` there, from inside a backward node: the
    second stream waits for what the current stream has been given so far, `reads` (the tensors `grads_fn` reads, allocated
    on the current stream) are marked for it, `grads_fn()` -> one gradient or None per entry of `params` runs on it, and
    the current stream re-joins at the end of the backward pass.  The caller decides whether its parameters are eligible
    (side_stream_enabled, can_publish) and returns None for them to autograd."""
    main = torch.cuda.current_stream()
    side = _side_stream(device)
    side.wait_stream(main)
    for t in reads:
        t.record_stream(side)
    with torch.cuda.stream(side):
        for param, g in zip(params, grads_fn()):
            if g is not None:
                _accumulate_grad(param, g, main)
    _join_later(main, side)


# ----------------------------------------------------------------------------- phase marks (dev instrumentation)
# tools/vae_phase_times.py sets MARKS = [] and reads (name, host time, event on the current stream) triples back; None
# (default) makes mark() a no-op.
MARKS = None


def mark(name: str) -> None:
    if MARKS is not None:
        import time
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        MARKS.append((name, time.perf_counter(), ev))


# ----------------------------------------------------------------------------- deferred parameter gradients
# The teacher-forced decoder uses the same parameters on every one of its ~20 steps, so a backward pass meets each
# Linear ~20 times.  Forming dW = dpre^T x (+ column sum, + the accumulate kernel autograd adds) per visit is ~40 tiny
# launches per parameter and pass.  With GGPM_DEFER_WGRADS=1 (default) a visit only queues its (dpre, x) rows; when the
# backward pass ends (autograd engine callback) every parameter gets ONE contraction over the stacked rows of all its
# visits -- dW = [dpre_1; dpre_2; ...]^T [x_1; x_2; ...], the same sum in a different order -- and other per-visit
# parameter gradients (the message functions', the embedding tables') are summed by one stacked reduction each.
# The queue is the one _DeferredGrads instance (_DEFERRED): nodes queue through _defer_linear / _defer_gather / _defer_sum;
# only its end-of-backward flush moves queued gradients into ``.grad``, on the stream they were queued on.


def defer_wgrads_enabled() -> bool:
    return os.environ.get("GGPM_DEFER_WGRADS", "1") != "0"


def _has_hooks(p) -> bool:
    return bool(getattr(p, "_backward_hooks", None)) or bool(getattr(p, "_post_accumulate_grad_hooks", None))


_PUBLISH = [True]


def publish_gradients(enabled: bool) -> bool:
    """Process-wide switch for gradients written to ``.grad`` by this package itself (deferred contractions, second
    stream, flat gradient buffer) instead of being returned through autograd.  -> the previous setting.

    Switch it OFF before wrapping a model in ``torch.nn.parallel.DistributedDataParallel`` or anything else that hooks the
    AccumulateGrad NODE of a parameter: such hooks live in the C++ node and cannot be seen from Python (``can_publish``
    only sees ``Tensor.register_hook`` and ``register_post_accumulate_grad_hook``), and a reducer whose hook never fires
    waits for a gradient that was written around it.  The data-parallel path this package supports and measures is
    ``ggpm_amd.parallel.FlatGradSync`` (one all-reduce of one flat buffer), which needs no hooks."""
    prev, _PUBLISH[0] = _PUBLISH[0], bool(enabled)
    return prev


def can_publish(*params) -> bool:
    """True when the gradients of these parameters may be written to ``.grad`` by this module itself (deferred
    contraction / second stream) instead of being returned through autograd: publishing is on (``publish_gradients``)
    and every parameter is a leaf that requires grad and carries NO Python-visible hook.  A parameter with a tensor hook
    or a post-accumulate-grad hook (hook-based clippers / reducers) gets its gradient the ordinary way, through
    AccumulateGrad, so that the hooks fire.  Hooks on the AccumulateGrad node itself (stock DDP's reducer) are not visible
    here: see ``publish_gradients``."""
    return _PUBLISH[0] and all(p is None or (getattr(p, "is_leaf", False) and p.requires_grad and not _has_hooks(p))
                               for p in params)


def _linear_grads(entries, use, target):
    """Every queued Linear's weight gradient (one contraction per K segment) and bias gradient in ONE library call
    (ggpm_linear_wgrads_batch: the same launches in the same order as ~60 separate gemm / colsum calls)."""
    items, keep, out, n_max, ws_max = [], [], [], 0, 0
    lib = _lib.load()
    for weight, bias, Ks, visits in entries:
        N = weight.shape[0]
        if len(visits) == 1:
            dpre, xs = use(visits[0][0]), [use(x) for x in visits[0][1]]
        else:
            dpre = torch.cat([use(v[0]) for v in visits], dim=0)
            xs = [torch.cat([use(v[1][i])[:, :K] for v in visits], dim=0) for i, K in enumerate(Ks)]
        M = dpre.shape[0]
        dW = target(weight)
        db = target(bias) if bias is not None else None
        o = 0
        for i, (x, K) in enumerate(zip(xs, Ks)):
            items.append((dpre.data_ptr(), _ld(dpre), x.data_ptr(), _ld(x), dW.data_ptr() + 4 * o, dW.stride(0),
                          db.data_ptr() if (db is not None and i == 0) else 0, M, N, K))
            ws_max = max(ws_max, int(lib.ggpm_gemm_workspace_bytes(N, K, M)))
            o += K
        n_max = max(n_max, N)
        keep.append((dpre, xs, dW, db))
        out.append((weight, dW))
        if db is not None:
            out.append((bias, db))
    if items:
        arr = _lib.array_type(WgradItem, len(items))(*[WgradItem(*it) for it in items])
        dev = keep[0][0].device
        ws = torch.empty(ws_max // 4, dtype=torch.float32, device=dev) if ws_max else None
        csws = torch.empty(256 * n_max, dtype=torch.float32, device=dev)
        _lib.check(lib.ggpm_linear_wgrads_batch(len(items), ctypes.addressof(arr), _p(ws), ws_max, _p(csws),
                                                _stream()), "linear_wgrads_batch")
    # handed out only now, behind the launch that writes them: an add into an existing .grad (gradient accumulation,
    # zero_grad(set_to_none=False), a Linear queued under two K splits) is enqueued after dW / db hold their values
    return out


def _sum_grads(entries, use, target):
    """One stacked reduction per parameter over its per-visit gradients (lazily: each is published before the next is formed)."""
    for param, grads in entries:
        yield param, use(grads[0]) if len(grads) == 1 else torch.stack([use(g) for g in grads], dim=0).sum(dim=0)


def _gather_grads(entries, use, target):
    """Embedding tables: d(table)[id] = sum of the rows that used id, one scatter per table (one at a time, as the sums)."""
    for table, width, visits in entries:
        dout = use(visits[0][0]) if len(visits) == 1 else torch.cat([use(v[0]) for v in visits], dim=0)
        idx = use(visits[0][1]) if len(visits) == 1 else torch.cat([use(v[1]).reshape(-1) for v in visits], dim=0)
        csrT = csr_from_index(idx.reshape(-1), ncols=table.shape[0]).T
        dtable = target(table)
        _segment_sum_raw(dout, csrT, width, dtable)
        yield table, dtable


class _DeferredGrads:
    """The deferred parameter gradients of ONE backward pass.  ``linear`` / ``sum`` / ``gather``: what is queued, by key;
    ``task``: the pass (autograd graph-task id) the end-of-backward flush is registered for, ``stream``: the stream its
    entries are queued on; ``early``: the other stream that wrote entries or formed ``pending``, the (param, grad) pairs
    of an early flush that wait for the end of the pass."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        """The one place the per-pass state is cleared."""
        self.linear, self.sum, self.gather = {}, {}, {}
        self.task = self.stream = self.early = None
        self.pending = []

    def _begin(self) -> None:
        """Queue the end-of-backward flush once per backward pass.  A pass is identified by the autograd engine's graph
        task id: a pass that RAISED never ran its callbacks, so whatever it left queued is dropped when the next pass
        registers (nothing sticky survives a failed backward)."""
        task = torch._C._current_graph_task_id()
        if self.task != task or task < 0:
            self.reset()
            self.task = task
            self.stream = torch.cuda.current_stream()
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def add_linear(self, weight, bias, dpre, xs, Ks) -> None:
        self._begin()
        # keyed by the parameter AND the column split it was visited with: a Linear used with two different K splits in one
        # pass gets one contraction per split (both land in the same .grad)
        key = (id(weight), tuple(Ks), id(bias) if bias is not None else 0)
        self.linear.setdefault(key, (weight, bias, tuple(Ks), []))[3].append((dpre, xs))

    def add_gather(self, table, width, dout, idx) -> None:
        self._begin()
        self.gather.setdefault((id(table), int(width)), (table, width, []))[2].append((dout, idx))

    def add_sum(self, param, grad) -> None:
        """param.grad += grad, summed with the pass's other contributions to the same parameter by ONE reduction at the end."""
        if grad is None:
            return
        self._begin()
        self.sum.setdefault(id(param), (param, []))[1].append(grad)

    def written_on(self, side: torch.cuda.Stream) -> None:
        """The entries queued so far were produced on `side`: the end-of-pass flush waits for it before it reads them."""
        self.early = side

    def flush(self, side: Optional[torch.cuda.Stream] = None) -> None:
        """Form the queued parameter gradients.  ``side`` = None: the end-of-backward callback, on the stream the entries
        were queued on.  ``side`` given (flush_early): on that stream, ordered behind everything the queueing stream has
        been given so far; the queueing stream re-joins at the end of the backward pass."""
        queues, main = (self.linear, self.sum, self.gather), self.stream
        if side is None:
            early, pending = self.early, self.pending
            self.reset()
            mark("bwd: end-of-pass flush starts")
            if main is not None and early is not None:
                # what the early flush computed on the second stream is handed to .grad HERE, on the queueing stream, once
                # that stream is ordered behind it: every mutation of .grad stays on one stream, whatever order the engine
                # ran the nodes in (autograd's own AccumulateGrad for tied / shared parameters included)
                main.wait_stream(early)
                with torch.cuda.stream(main):
                    for param, g in pending:
                        _accumulate_grad(param, g, main)
        else:
            self.linear, self.sum, self.gather = {}, {}, {}
        if not any(queues) or main is None:
            return
        stream = main
        if side is not None:
            side.wait_stream(main)
            stream = self.early = side

        def use(t):                        # queued on one stream, read on another: keep the allocator from recycling it early
            if side is not None and isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(stream)
            return t

        def target(param):
            """Where a parameter's gradient is formed: its slice of the flat gradient buffer (parallel.FlatGradSync) when it has
            one and nothing has been written there in this pass -- the optimizer / all-reduce side then finds it in place (no
            pack copy: one multi-tensor launch right in front of the optimizer, and ~35 `.grad` re-pointings, less per step) --
            else a fresh tensor.  The first contribution of a pass writes, later ones are added (`_accumulate_grad`)."""
            v = grad_view(param)
            if v is not None and id(param) not in taken:
                taken.add(id(param))
                return v
            return torch.empty_like(param)

        taken = set(id(q) for q, _ in self.pending)
        with torch.cuda.stream(stream):
            for step, queue in zip((_linear_grads, _sum_grads, _gather_grads), queues):
                for param, g in step(queue.values(), use, target):
                    if side is not None:   # computed early: published by the end-of-backward flush (see above)
                        self.pending.append((param, g))
                    else:
                        _accumulate_grad(param, g, main)

    def flush_early(self) -> None:
        """Called from inside a backward pass at a point after which only nodes WITHOUT deferred gradients have much left to
        do (the decoder's atom level and the encoder, once the heads and the tree-side levels have run): the queued
        contractions start now on the second stream, beside that work, instead of behind it.  Whatever is queued later still
        goes through the end-of-backward flush.  _dev.DEFER_EARLY = False switches it off."""
        if not _dev.DEFER_EARLY or not side_stream_enabled():
            return
        if self.stream is None or self.task is None or self.task != torch._C._current_graph_task_id():
            return
        self.flush(side=_side_stream(self.stream.device))   # (the end-of-backward callback stays registered: it publishes)


_DEFERRED = _DeferredGrads()
_defer_linear, _defer_gather, _defer_sum = _DEFERRED.add_linear, _DEFERRED.add_gather, _DEFERRED.add_sum
flush_deferred_early = _DEFERRED.flush_early


# ----------------------------------------------------------------------------- GRU / LSTM cell adapters
# Everything the host side knows about ONE message function: the order of its parameter tuple, its (W, b) gate pairs, the
# hidden halves of its weights, which gate-input plane its backward re-reads, its stash set, and how the ten level entry
# points of the C ABI (ggpm_{gru,lstm}_{forward,backward,weight_grads,sparse_forward,sparse_backward}) take all of that.
# The autograd nodes below, tree_decode.py and atom_decode.py are written once against this surface; the adapters are the
# only place in the package where those entry points are called.  A node builds one adapter per call (never per decode
# step); building one is a tuple unpack.
def _a(v) -> ctypes.c_void_p:
    """A device argument of a level call: a tensor, None, or a raw address (the atom-level plan hands out addresses into
    its packed upload)."""
    return ctypes.c_void_p(v if isinstance(v, int) else 0 if v is None else v.data_ptr())


def _csr_args(csr):
    """(rowptr, col) arguments from a CSR or a (rowptr, col) pair of device arguments"""
    rowptr, col = (csr.rowptr, csr.col) if isinstance(csr, CSR) else csr
    return _a(rowptr), _a(col)


class _Cell:
    """What GruCell and LstmCell share.  ``params``: the cell's parameters in the order rnn.GRU / rnn.LSTM hand them to
    ``gru_level`` / ``lstm_level`` (``level_params()``); ``gates``: the (W [H, I + H], b) pairs in the order of the
    gate-input planes X[0..G-1].  ``dW_hidden`` of the backward calls is ``dW_buffers()[1]``: the hidden-half gradients."""
    G = reread = None           # number of gates; index of the gate-input plane the backward re-reads
    U_r = b_u = None            # GRU only: W_r has no hidden half, U_r [H, H] is its own matrix (with the cell's bias b_u)

    def __init__(self, params, I: int, H: int):
        self.params, self.I, self.H, self.Hp = tuple(params), I, H, padded_hidden(H)

    lib = property(lambda self: _lib.load())

    @property
    def weights(self):
        """the matrices among ``params`` (what a node saves for its backward)"""
        return tuple(p for p in self.params if p.dim() == 2)

    def _f32(self):
        return dict(dtype=torch.float32, device=self.params[0].device)

    def hidden(self):
        """[(hidden-half view or U_r, leading dimension)] in the order the depth kernels take them"""
        return [(W[:, self.I:], W.stride(0)) for W, _ in self.gates]

    def hidden_weight_arrays(self):
        """-> (c_void_p * 4, c_int * 4): ``hidden()`` as the decode driver takes it"""
        hw = self.hidden()
        return (_lib.array_type(ctypes.c_void_p, 4)(*[w.data_ptr() for w, _ in hw]),
                _lib.array_type(ctypes.c_int, 4)(*[ld for _, ld in hw]))

    def _weight_args(self, backward: bool):
        return [v for w, ld in self.hidden() for v in (_a(w), ld)]

    def _lds(self, hid, ld_dW):
        return [ld_dW if ld_dW is not None else t.stride(0) for t in hid[:self.G]]

    # ---- gate inputs
    def project_inputs(self, x, ldx: int, rows: int, X) -> None:
        """X[k][:rows] = x W_k[:, :I]^T + b_k: the hoisted input GEMMs (depth invariant)"""
        for k, (W, b) in enumerate(self.gates):
            gemm(0, 1, rows, self.H, self.I, x, ldx, W, W.stride(0), X[k], self.Hp, self.Hp, bias=b)

    def input_grad(self, dX, x, rows: int) -> torch.Tensor:
        """-> dx = sum_k dX_k W_k[:, :I], in x's layout"""
        dx = _empty_same_layout(x)
        for k, (W, _) in enumerate(self.gates):
            gemm(0, 0, rows, self.I, self.H, dX[k], self.Hp, W, W.stride(0), dx, _ld(x), x.shape[1] if k == 0 else self.I,
                 accumulate=k > 0)
        return dx

    def bias_grads(self, dX, rows: int) -> list:
        """-> [db_k = column sums of dX_k, or None where the gate has no bias (W_r)]"""
        return [colsum(dX[k], rows, self.H) if b is not None else None for k, (_, b) in enumerate(self.gates)]

    def input_half_grads(self, dX, x, ldx: int, rows: int, bufs, interleaved: Optional[bool] = None) -> list:
        """bufs[k][:, :I] = dX_k^T x; -> ``bias_grads``.  The launch order is the one every form has always had:
        ``interleaved`` (each gate's column sum right behind its GEMM) is the LSTM nodes' and the tree level's, all GEMMs
        first the GRU nodes'."""
        H, I, Hp = self.H, self.I, self.Hp
        interleaved = self.G == 4 if interleaved is None else interleaved
        dbs = []
        for k, (dW, (_, b)) in enumerate(zip(bufs, self.gates)):
            gemm(1, 0, H, I, rows, dX[k], Hp, x, ldx, dW, dW.stride(0), I, splitk=True)
            if interleaved:
                dbs.append(colsum(dX[k], rows, H) if b is not None else None)
        return dbs if interleaved else self.bias_grads(dX, rows)

    # ---- buffers
    def alloc_state(self, rows: int, depth: int, save: bool):
        """-> Hs, Cs, Qs, St.  ``save``: every depth slot, for a backward; else two ping-pong slots and no stashes."""
        f32, n = self._f32(), (depth + 1 if save else 2)
        Hs = torch.empty(n, rows, self.Hp, **f32)
        Cs = torch.empty(n, rows, self.Hp, **f32) if self.G == 4 else None
        Qs = torch.empty(depth if save else 2, rows, self.Hp, **f32)
        return Hs, Cs, Qs, (torch.empty(5, depth, rows, self.Hp, **f32) if save else (None,) * 5)

    def alloc_pack(self) -> torch.Tensor:
        return torch.empty(self.pack_floats(), **self._f32())

    def dW_buffers(self):
        """-> (one [H, I + H] gradient buffer per gate weight, the hidden-half gradients the backward calls write: views of
        those buffers' columns [I, I + H); GruCell: Wz_h, U_r, Wh_h, b_u, with U_r and b_u their own tensors)"""
        bufs = [torch.empty(W.shape, **self._f32()) for W, _ in self.gates]
        return bufs, [b[:, self.I:] for b in bufs]


class GruCell(_Cell):
    """GRU (ggpm/rnn.py:5-59); params (W_z, b_z, W_r, U_r, b_u, W_h, b_h); planes X_z, X_r, X_h; stashes S, G, Z, M, R"""
    G, reread = 3, 1

    def __init__(self, params, I: int, H: int):
        super().__init__(params, I, H)
        W_z, b_z, W_r, self.U_r, self.b_u, W_h, b_h = self.params
        self.gates = ((W_z, b_z), (W_r, None), (W_h, b_h))

    def hidden(self):
        (W_z, _), _, (W_h, _) = self.gates
        return [(W_z[:, self.I:], W_z.stride(0)), (self.U_r, self.U_r.stride(0)), (W_h[:, self.I:], W_h.stride(0))]

    def _weight_args(self, backward: bool):
        (wz, ld_z), (ur, ld_u), (wh, ld_h) = self.hidden()
        return (_a(wz), ld_z, _a(ur), ld_u) + (() if backward else (_a(self.b_u),)) + (_a(wh), ld_h)

    def _dW_args(self, hid, ld_dW):
        ld = self._lds(hid, ld_dW)
        return _a(hid[0]), ld[0], _a(hid[1]), ld[1], _a(hid[3]), _a(hid[2]), ld[2]

    def dW_buffers(self):
        bufs, hid = super().dW_buffers()
        f32 = self._f32()
        return bufs, [hid[0], torch.empty(self.H, self.H, **f32), hid[2], torch.empty(self.H, **f32)]

    def grads(self, bufs, hid, dbs) -> tuple:
        """-> the gradients in ``params`` order from the gate buffers, the hidden-half list and ``bias_grads``"""
        return bufs[0], dbs[0], bufs[1], hid[1], hid[3], bufs[2], dbs[2]

    def pack_floats(self) -> int:
        return int(self.lib.ggpm_gru_pack_floats(self.H))

    def backward_workspace(self, rows: int, depth: int) -> torch.Tensor:
        wb = int(self.lib.ggpm_gru_backward_workspace_bytes(rows, self.H, depth))
        return torch.empty((wb + 3) // 4, **self._f32())

    def forward(self, *, rows, depth, X, pred, Hs, Qs, St, wpack, save, Cs=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_gru_forward(
            rows, self.H, depth, *map(_a, X), *self._weight_args(False), *_csr_args(pred), _a(Hs), _a(Qs), *map(_a, St),
            _a(wpack), int(save), opts, _stream() if stream is None else stream), "gru_forward")

    def sparse_forward(self, *, rows, depth, h_in, frozen, X, pred, Hs, Qs, St, wpack, save, c_in=None, Cs=None, opts=None,
                       stream=None):
        _lib.check(self.lib.ggpm_gru_sparse_forward(
            rows, self.H, depth, _a(h_in), _a(frozen), *map(_a, X), *self._weight_args(False), *_csr_args(pred), _a(Hs),
            _a(Qs), *map(_a, St), _a(wpack), int(save), opts, _stream() if stream is None else stream), "gru_sparse_forward")

    def backward(self, *, rows, depth, Xg, pred, succ, Hs, Qs, St, d_out, dX, dW_hidden, work, weight_grads, Cs=None,
                 ld_dW=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_gru_backward(
            rows, self.H, depth, _a(Xg), *self._weight_args(True), *_csr_args(pred), *_csr_args(succ), _a(Hs), _a(Qs),
            *map(_a, St), _a(d_out), *map(_a, dX), *self._dW_args(dW_hidden, ld_dW), _a(work), work.numel() * 4,
            int(weight_grads), opts, _stream() if stream is None else stream), "gru_backward")

    def weight_grads(self, *, rows, depth, Hs, St, work, dW_hidden, ld_dW=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_gru_weight_grads(
            rows, self.H, depth, _a(Hs), _a(St[0]), _a(St[1]), _a(work), work.numel() * 4, *self._dW_args(dW_hidden, ld_dW),
            opts, _stream() if stream is None else stream), "gru_weight_grads")

    def sparse_backward(self, *, rows, depth, frozen, Xg, pred, succ, Hs, Qs, St, d_out, d_in, dX, dW_hidden, work, Cs=None,
                        dc_out=None, dc_in=None, ld_dW=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_gru_sparse_backward(
            rows, self.H, depth, _a(frozen), _a(Xg), *self._weight_args(True), *_csr_args(pred), *_csr_args(succ), _a(Hs),
            _a(Qs), *map(_a, St), _a(d_out), _a(d_in), *map(_a, dX), *self._dW_args(dW_hidden, ld_dW), _a(work),
            work.numel() * 4, opts, _stream() if stream is None else stream), "gru_sparse_backward")


class LstmCell(_Cell):
    """LSTM (ggpm/rnn.py:61-121); params (W_i, b_i, W_o, b_o, W_u, b_u, W_f, b_f); planes X_i, X_o, X_u, X_f; stashes S, I,
    O, U, F; carries the cell state (Cs, c_in, dc_out, dc_in) beside the hidden state"""
    G, reread = 4, 3

    def __init__(self, params, I: int, H: int):
        super().__init__(params, I, H)
        p = self.params
        self.gates = ((p[0], p[1]), (p[2], p[3]), (p[4], p[5]), (p[6], p[7]))

    def _dW_args(self, hid, ld_dW):
        return [v for t, ld in zip(hid, self._lds(hid, ld_dW)) for v in (_a(t), ld)]

    def grads(self, bufs, hid, dbs) -> tuple:
        """-> the gradients in ``params`` order from the gate buffers and ``bias_grads`` (``hid``: views of ``bufs``)"""
        return tuple(g for pair in zip(bufs, dbs) for g in pair)

    def pack_floats(self) -> int:
        return int(self.lib.ggpm_lstm_pack_floats(self.H))

    def backward_workspace(self, rows: int, depth: int) -> torch.Tensor:
        wb = int(self.lib.ggpm_lstm_backward_workspace_bytes(rows, self.H, depth))
        return torch.empty((wb + 3) // 4, **self._f32())

    def forward(self, *, rows, depth, X, pred, Hs, Cs, Qs, St, wpack, save, opts=None, stream=None):
        _lib.check(self.lib.ggpm_lstm_forward(
            rows, self.H, depth, *map(_a, X), *self._weight_args(False), *_csr_args(pred), _a(Hs), _a(Cs), _a(Qs),
            *map(_a, St), _a(wpack), int(save), opts, _stream() if stream is None else stream), "lstm_forward")

    def sparse_forward(self, *, rows, depth, h_in, c_in, frozen, X, pred, Hs, Cs, Qs, St, wpack, save, opts=None, stream=None):
        _lib.check(self.lib.ggpm_lstm_sparse_forward(
            rows, self.H, depth, _a(h_in), _a(c_in), _a(frozen), *map(_a, X), *self._weight_args(False), *_csr_args(pred),
            _a(Hs), _a(Cs), _a(Qs), *map(_a, St), _a(wpack), int(save), opts, _stream() if stream is None else stream),
            "lstm_sparse_forward")

    def backward(self, *, rows, depth, Xg, pred, succ, Hs, Cs, Qs, St, d_out, dX, dW_hidden, work, weight_grads, ld_dW=None,
                 opts=None, stream=None):
        _lib.check(self.lib.ggpm_lstm_backward(
            rows, self.H, depth, _a(Xg), *self._weight_args(True), *_csr_args(pred), *_csr_args(succ), _a(Hs), _a(Cs),
            _a(Qs), *map(_a, St), _a(d_out), *map(_a, dX), *self._dW_args(dW_hidden, ld_dW), _a(work), work.numel() * 4,
            int(weight_grads), opts, _stream() if stream is None else stream), "lstm_backward")

    def weight_grads(self, *, rows, depth, Hs, St, work, dW_hidden, ld_dW=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_lstm_weight_grads(
            rows, self.H, depth, _a(Hs), _a(St[0]), _a(work), work.numel() * 4, *self._dW_args(dW_hidden, ld_dW), opts,
            _stream() if stream is None else stream), "lstm_weight_grads")

    def sparse_backward(self, *, rows, depth, frozen, Xg, pred, succ, Hs, Cs, Qs, St, d_out, dc_out, d_in, dc_in, dX,
                        dW_hidden, work, ld_dW=None, opts=None, stream=None):
        _lib.check(self.lib.ggpm_lstm_sparse_backward(
            rows, self.H, depth, _a(frozen), _a(Xg), *self._weight_args(True), *_csr_args(pred), *_csr_args(succ), _a(Hs),
            _a(Cs), _a(Qs), *map(_a, St), _a(d_out), _a(dc_out), _a(d_in), _a(dc_in), *map(_a, dX),
            *self._dW_args(dW_hidden, ld_dW), _a(work), work.numel() * 4, opts, _stream() if stream is None else stream),
            "lstm_sparse_backward")


def cell_for(lstm: bool, params, I: int, H: int) -> _Cell:
    return (LstmCell if lstm else GruCell)(params, I, H)


# ----------------------------------------------------------------------------- dense levels
def _level_forward(ctx, cell: _Cell, x, pred: CSR, depth: int, gate_dtype: int):
    """GRU.forward / LSTM.forward (ggpm/rnn.py:41-50, 96-108) for one level: hoisted input GEMMs + fused depth loop.
    -> (h_D, c_D or None) as [E1, Hp] tensors (pad columns zero)."""
    _need_gpu(x, *cell.params)
    E1 = x.shape[0]
    save = any(ctx.needs_input_grad)
    X = torch.empty(cell.G, E1, cell.Hp, dtype=torch.float32, device=x.device)
    cell.project_inputs(x, _ld(x), E1, X)
    wpack = cell.alloc_pack()
    Hs, Cs, Qs, St = cell.alloc_state(E1, depth, save)
    cell.forward(rows=E1, depth=depth, X=X, pred=pred, Hs=Hs, Cs=Cs, Qs=Qs, St=St, wpack=wpack, save=save,
                 opts=_gate_opts(gate_dtype))
    k = depth if save else depth & 1
    if save:
        ctx.save_for_backward(x, *cell.weights)
        ctx.stash = (X[cell.reread], Hs, Cs, Qs, St)
        ctx.meta = (cell, pred, depth, gate_dtype)
    return Hs[k], (Cs[k] if Cs is not None else None)


def _level_backward(ctx, dHD, name: str):
    """One autograd node per level: the backward writes the x-half and the h-half gradient of every gate weight straight
    into ONE full-shape gradient tensor (no slice/cat/add kernels from autograd).
    -> the gradients of (x, pred, depth, I, H, gate_dtype, *params)"""
    x = ctx.saved_tensors[0]
    if ctx.stash is None:
        raise second_backward(name)
    Xg, Hs, Cs, Qs, St = ctx.stash
    cell, pred, depth, gate_dtype = ctx.meta
    E1 = x.shape[0]
    succ = pred.T
    dHD = dHD.contiguous()
    dX = torch.empty(cell.G, E1, cell.Hp, dtype=torch.float32, device=x.device)
    bufs, hid = cell.dW_buffers()
    work = cell.backward_workspace(E1, depth)
    use_side = side_stream_enabled() and can_publish(*cell.params)
    cell.backward(rows=E1, depth=depth, Xg=Xg, pred=pred, succ=succ, Hs=Hs, Cs=Cs, Qs=Qs, St=St, d_out=dHD, dX=dX,
                  dW_hidden=hid, work=work, weight_grads=not use_side, opts=_gate_opts(gate_dtype))
    ctx.stash = None
    dx = cell.input_grad(dX, x, E1) if ctx.needs_input_grad[0] else None     # needed upstream right away: main stream

    def weight_grads():
        if use_side:
            cell.weight_grads(rows=E1, depth=depth, Hs=Hs, St=St, work=work, dW_hidden=hid, opts=_gate_opts(gate_dtype))
        # x-halves of the gate weights and the gate biases
        return cell.grads(bufs, hid, cell.input_half_grads(dX, x, _ld(x), E1, bufs))

    if use_side:
        publish_aside(x.device, (work, dX, Hs, St, x, *bufs, *hid), cell.params, weight_grads)
        return (dx,) + (None,) * (5 + len(cell.params))
    return (dx, None, None, None, None, None, *weight_grads())


class _GruLevel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pred, depth, I, H, gate_dtype, *params):
        return _level_forward(ctx, GruCell(params, I, H), x, pred, depth, gate_dtype)[0]

    @staticmethod
    def backward(ctx, dHD):
        return _level_backward(ctx, dHD, "gru_level")


class _LstmLevel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pred, depth, I, H, gate_dtype, *params):
        h, c = _level_forward(ctx, LstmCell(params, I, H), x, pred, depth, gate_dtype)
        ctx.mark_non_differentiable(c)
        return h, c

    @staticmethod
    def backward(ctx, dHD, _dC):
        return _level_backward(ctx, dHD, "lstm_level")


GATE_DTYPES = {"f32": 0, "fp32": 0, "bf16": 1, "f32_mfma": 2, "f32_split": 3, None: 0, 0: 0, 1: 1, 2: 2, 3: 3}


def gru_level(x, W_z, b_z, W_r, U_r, b_u, W_h, b_h, pred: CSR, depth: int, I: int, H: int, gate_dtype=None) -> torch.Tensor:
    return _GruLevel.apply(x, pred, depth, I, H, GATE_DTYPES[gate_dtype], W_z, b_z, W_r, U_r, b_u, W_h, b_h)


def lstm_level(x, W_i, b_i, W_o, b_o, W_u, b_u, W_f, b_f, pred: CSR, depth: int, I: int, H: int, gate_dtype=None):
    return _LstmLevel.apply(x, pred, depth, I, H, GATE_DTYPES[gate_dtype], W_i, b_i, W_o, b_o, W_u, b_u, W_f, b_f)


# ----------------------------------------------------------------------------- sparse (incremental) levels
def _as_padded_state(h: torch.Tensor, H: int, Hp: int) -> torch.Tensor:
    """[E, H] public state -> [E, Hp] buffer with zero pad columns (no copy when it already is a view of one)."""
    if h.dim() == 2 and h.shape[1] == H and h.stride(1) == 1 and h.stride(0) == Hp and Hp != H \
            and h.storage_offset() % Hp == 0:
        return h.as_strided((h.shape[0], Hp), (Hp, 1), h.storage_offset())     # our own earlier output
    if Hp == H:
        return h.contiguous()
    out = torch.zeros(h.shape[0], Hp, dtype=h.dtype, device=h.device)
    out[:, :H] = h
    return out


def _scatter_rows(full_rows: int, sub: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """zeros([full_rows, ...]) with rows `index` := sub (the subset tensors of get_sub_tensor back in place)."""
    out = torch.zeros((full_rows,) + tuple(sub.shape[1:]), dtype=sub.dtype, device=sub.device)
    out.index_copy_(0, index, sub)
    return out


def _sparse_structure(E1: int, submess: torch.Tensor, bgraph_sub: torch.Tensor):
    """(frozen mask [E1] uint8, predecessor CSR over all E1 rows) of a sparse_forward call, remembered on ``bgraph_sub``."""
    key = (E1, submess.data_ptr(), submess.numel(), version_of(submess))
    hit = _memo_get(bgraph_sub, "_ggpm_sparse", key)
    if hit is not None:
        return hit
    frozen = torch.ones(E1, dtype=torch.uint8, device=submess.device)
    frozen.index_fill_(0, submess, 0)
    pred = csr_from_padded(_scatter_rows(E1, bgraph_sub, submess), ncols=E1)
    return _memo_put(bgraph_sub, "_ggpm_sparse", key, (frozen, pred, submess))      # (keeps `submess` alive: the key names it)


def _sparse_forward(ctx, cell: _Cell, h_in, c_in, x_sub, submess, bgraph_sub, depth: int):
    """GRU.sparse_forward / LSTM.sparse_forward (ggpm/rnn.py:52-59, 110-121): recompute the rows `submess` of the message
    state `depth` times.  -> (h [E1, H], c [E1, H] or None)"""
    _need_gpu(h_in, c_in, x_sub, submess, bgraph_sub, cell.params[0])
    H, Hp = cell.H, cell.Hp
    E1, ms = h_in.shape[0], submess.numel()
    f32 = dict(dtype=torch.float32, device=h_in.device)
    save = any(ctx.needs_input_grad)
    hp = _as_padded_state(h_in, H, Hp)
    cp = _as_padded_state(c_in, H, Hp) if c_in is not None else None
    frozen, pred, _ = _sparse_structure(E1, submess, bgraph_sub)
    Xs = torch.empty(cell.G, ms, Hp, **f32)
    cell.project_inputs(x_sub, _ld(x_sub), ms, Xs)
    X = torch.zeros(cell.G, E1, Hp, **f32)
    X.index_copy_(1, submess, Xs)
    wpack = cell.alloc_pack()
    Hs, Cs, Qs, St = cell.alloc_state(E1, depth, save)
    cell.sparse_forward(rows=E1, depth=depth, h_in=hp, c_in=cp, frozen=frozen, X=X, pred=pred, Hs=Hs, Cs=Cs, Qs=Qs, St=St,
                        wpack=wpack, save=save)
    k = depth if save else depth & 1
    if save:
        ctx.save_for_backward(x_sub, submess, *cell.weights)
        ctx.stash = (X[cell.reread], frozen, pred, Hs, Cs, Qs, St)
        ctx.meta = (cell, depth)
    return Hs[k][:, :H], (Cs[k][:, :H] if Cs is not None else None)


def _sparse_backward(ctx, dH, dC, want_dx: bool, name: str):
    """-> (dh_in, dc_in or None, dx_sub or None, the parameter gradients: None where they were queued for the pass's end)"""
    x_sub, submess = ctx.saved_tensors[:2]
    if ctx.stash is None:
        raise second_backward(name)
    Xg, frozen, pred, Hs, Cs, Qs, St = ctx.stash
    cell, depth = ctx.meta
    H, Hp = cell.H, cell.Hp
    E1, ms = Hs.shape[1], submess.numel()
    f32 = dict(dtype=torch.float32, device=x_sub.device)
    lstm = Cs is not None
    succ = pred.T
    dHD = torch.zeros(E1, Hp, **f32)
    dCD = torch.zeros(E1, Hp, **f32) if lstm else None
    if dH is not None:
        dHD[:, :H] = dH
    if dC is not None:
        dCD[:, :H] = dC
    dHin = torch.empty(E1, Hp, **f32)
    dCin = torch.empty(E1, Hp, **f32) if lstm else None
    dX = torch.empty(cell.G, E1, Hp, **f32)
    bufs, hid = cell.dW_buffers()
    work = cell.backward_workspace(E1, depth)
    cell.sparse_backward(rows=E1, depth=depth, frozen=frozen, Xg=Xg, pred=pred, succ=succ, Hs=Hs, Cs=Cs, Qs=Qs, St=St,
                         d_out=dHD, dc_out=dCD, d_in=dHin, dc_in=dCin, dX=dX, dW_hidden=hid, work=work)
    ctx.stash = None
    dXs = dX.index_select(1, submess)             # [G, ms, Hp]: only the recomputed rows carry input gradients
    pgrads = cell.grads(bufs, hid, cell.input_half_grads(dXs, x_sub, _ld(x_sub), ms, bufs))
    dx = cell.input_grad(dXs, x_sub, ms) if want_dx else None
    if defer_wgrads_enabled() and can_publish(*cell.params):
        for q, g in zip(cell.params, pgrads):         # summed once per parameter at the end of the pass (see _DeferredGrads)
            _defer_sum(q, g)
        pgrads = (None,) * len(pgrads)
    return dHin[:, :H], (dCin[:, :H] if lstm else None), dx, pgrads


class _GruSparse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h_in, x_sub, submess, bgraph_sub, depth, I, H, *params):
        return _sparse_forward(ctx, GruCell(params, I, H), h_in, None, x_sub, submess, bgraph_sub, depth)[0]

    @staticmethod
    def backward(ctx, dH):
        dh, _, dx, pgrads = _sparse_backward(ctx, dH, None, ctx.needs_input_grad[1], "gru_sparse")
        return (dh, dx, None, None, None, None, None, *pgrads)


class _LstmSparse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h_in, c_in, x_sub, submess, bgraph_sub, depth, I, H, *params):
        return _sparse_forward(ctx, LstmCell(params, I, H), h_in, c_in, x_sub, submess, bgraph_sub, depth)

    @staticmethod
    def backward(ctx, dH, dC):
        dh, dc, dx, pgrads = _sparse_backward(ctx, dH, dC, ctx.needs_input_grad[2], "lstm_sparse")
        return (dh, dc, dx, None, None, None, None, None, *pgrads)


def gru_sparse(h_in, x_sub, submess, bgraph_sub, W_z, b_z, W_r, U_r, b_u, W_h, b_h, depth: int, I: int, H: int):
    return _GruSparse.apply(h_in, x_sub, submess, bgraph_sub, depth, I, H, W_z, b_z, W_r, U_r, b_u, W_h, b_h)


def lstm_sparse(h_in, c_in, x_sub, submess, bgraph_sub, W_i, b_i, W_o, b_o, W_u, b_u, W_f, b_f, depth, I, H):
    return _LstmSparse.apply(h_in, c_in, x_sub, submess, bgraph_sub, depth, I, H, W_i, b_i, W_o, b_o, W_u, b_u, W_f, b_f)
