"""numpy fp64 restatement of the two operations the STL / DReG estimators of ``bound_loss(objective="iwae")`` add
(include/ggpm_hip.h, *Path-derivative estimators of the importance-weighted bound*): the normalised importance weights with
their effective sample size, and the backward of the latent terms with the parameters of log q held fixed.
tests/test_mol_estimator_cpu.py checks the formulas here against torch fp64 autograd of the surrogate loss, for unbiasedness on
a toy model and at the true posterior; the GPU tests compare the kernels with these."""
import numpy as np

from mol_objective_oracle import nll_of


def iwae_weights(parts, logpq):
    """parts [K, B, 4], logpq [K, B] -> (s [K, B] = softmax_k(logpq - nll), ess [B] = 1 / sum_k s^2)"""
    lw = np.asarray(logpq, np.float64) - nll_of(parts)
    e = np.exp(lw - lw.max(axis=0)[None])
    s = e / e.sum(axis=0)[None]
    return s, 1.0 / (s * s).sum(axis=0)


def latent_terms_backward_path(dz, mean, pre_var, eps, c_logpq, s=None, g=1.0):
    """-> (dmean [B, L], dpre_var [B, L]): with G = g c_logpq, t = dz - G z, a = t + G eps exp(-lv / 2), q = s (None: 1),
    dmean = sum_k q a, dlv = sum_k q (t sd eps / 2 + G eps^2 / 2).  A sample with G eps = 0 adds no exp(-lv / 2) term."""
    m, p, e = (np.asarray(a, np.float64) for a in (mean, pre_var, eps))
    K, B, L = e.shape
    dz = np.zeros((K, B, L)) if dz is None else np.asarray(dz, np.float64)
    G = g * (np.zeros((K, B)) if c_logpq is None else np.asarray(c_logpq, np.float64))[:, :, None]
    q = np.ones((K, B, 1)) if s is None else np.asarray(s, np.float64)[:, :, None]
    lv = -np.abs(p)
    sd = np.exp(lv / 2)
    z = m[None] + sd[None] * e
    t = dz - G * z
    Ge = G * e
    with np.errstate(over="ignore", invalid="ignore"):
        path = np.where(Ge != 0.0, Ge * np.exp(-lv / 2)[None], 0.0)
    dmean = (q * (t + path)).sum(axis=0)
    dlv = (q * (t * (0.5 * sd[None] * e) + 0.5 * Ge * e)).sum(axis=0)
    return dmean, -np.sign(p) * dlv
