"""numpy fp64 restatement of the per-dimension entries (include/ggpm_hip.h, *The latent column by column*): the accumulator
and its finish, the free-bits KL, its gradient, and the free-bits loss of ``bound_loss(free_bits=...)``.  The reference has no
free bits, so this restatement is the yardstick; tests/test_latent_dims_cpu.py checks it against central differences, against
tests/mol_objective_oracle.py at lambda = 0 and against numpy.var."""
import numpy as np

ROWS = 5


def kl_dim(mean, pre_var):
    """[B, L]: -0.5 (1 + lv - mean^2 - exp(lv)), lv = -|pre_var|"""
    m, p = np.asarray(mean, np.float64), np.asarray(pre_var, np.float64)
    lv = -np.abs(p)
    return -0.5 * (1.0 + lv - m * m - np.exp(lv))


def accumulate(mean, pre_var, acc=None):
    """-> acc [5, L] with the batch's count and column sums of mean, mean^2, exp(lv) and kl_dim added (a new array)"""
    m, p = np.asarray(mean, np.float64), np.asarray(pre_var, np.float64)
    B, L = m.shape
    acc = np.zeros((ROWS, L)) if acc is None else np.array(acc, np.float64)
    acc[0] += B
    acc[1] += m.sum(axis=0)
    acc[2] += (m * m).sum(axis=0)
    acc[3] += np.exp(-np.abs(p)).sum(axis=0)
    acc[4] += kl_dim(m, p).sum(axis=0)
    return acc


def finish(acc, au_threshold):
    """-> (out [5, L]: kl_dims, mu_mean, mu_var, sigma2_mean, agg_var; n_active)"""
    acc = np.asarray(acc, np.float64)
    L = acc.shape[1]
    out = np.zeros((ROWS, L))
    n = acc[0]
    ok = n > 0
    d = np.where(ok, n, 1.0)
    out[0] = np.where(ok, acc[4] / d, 0.0)
    out[1] = np.where(ok, acc[1] / d, 0.0)
    out[2] = np.where(ok, np.maximum(acc[2] / d - out[1] * out[1], 0.0), 0.0)
    out[3] = np.where(ok, acc[3] / d, 0.0)
    out[4] = out[2] + out[3]
    return out, int((out[2] > au_threshold).sum())


def klbar(mean, pre_var, w=None):
    """[L]: (1/B) sum_b w_b kl_dim[b, j]"""
    kd = kl_dim(mean, pre_var)
    B = kd.shape[0]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    return (w[:, None] * kd).sum(axis=0) / B


def free_bits_kl(mean, pre_var, w, lam):
    """-> (kl_dims [L], term): term = sum_j max(lam, klbar_j)"""
    kb = klbar(mean, pre_var, w)
    return kb, np.maximum(float(lam), kb).sum()


def free_bits_kl_backward(mean, pre_var, w, lam, g=1.0):
    """-> (dmean [B, L], dpre_var [B, L]) of g * term; a column with klbar_j <= lam is free (strict >)"""
    m, p = np.asarray(mean, np.float64), np.asarray(pre_var, np.float64)
    B = m.shape[0]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    gate = klbar(m, p, w) > float(lam)
    c = np.where(gate[None, :], g * w[:, None] / B, 0.0)
    dlv = -0.5 * c * (1.0 - np.exp(-np.abs(p)))
    return c * m, -np.sign(p) * dlv


def free_bits_loss(nll, mean, pre_var, w, beta, lam):
    """(1/B) sum_i w_i (1/K) sum_k nll[k, i] + beta sum_j max(lam, klbar_j)"""
    nll = np.asarray(nll, np.float64)
    B = nll.shape[1]
    ww = np.ones(B) if w is None else np.asarray(w, np.float64)
    return (ww * nll.mean(axis=0)).sum() / B + beta * free_bits_kl(mean, pre_var, w, lam)[1]
