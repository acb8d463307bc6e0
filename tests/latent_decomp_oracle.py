"""numpy fp64 restatement of the KL split across the batch (include/ggpm_hip.h, *The KL split across the batch*): the forward
(index-code mutual information, total correlation, dimension-wise KL by minibatch-weighted sampling), its backward, the
accumulator and the beta-TCVAE loss of ``bound_loss(objective="tcvae")`` with its gradient chained through the rsample.  The
reference has no such split, so this restatement is the yardstick; tests/test_latent_decomp_cpu.py checks it against torch
autograd in fp64."""
import numpy as np

ROWS = 4
LOG_2PI = float(np.log(2.0 * np.pi))


def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.exp(a - m).sum(axis=axis))


def ell(z, mean, pre_var):
    """[K, B, B, L]: log N(z[k, i, l]; mean[j, l], exp(lv[j, l])), lv = -|pre_var|"""
    z, m, p = np.asarray(z, np.float64), np.asarray(mean, np.float64), np.asarray(pre_var, np.float64)
    lv = -np.abs(p)
    d = z[:, :, None, :] - m[None, None, :, :]
    return -0.5 * (LOG_2PI + lv[None, None] + d * d * np.exp(-lv)[None, None])


def log_nb(dataset_size, B):
    return float(np.log(float(dataset_size) * float(B)))


def forward(z, mean, pre_var, c):
    """-> dict(mi, tc, dwkl [K, B], dwkl_dim [K, B, L], A [K, B], D [K, B, L], S [K, B, B], p [K, B, B])"""
    z = np.asarray(z, np.float64)
    K, B, L = z.shape
    e = ell(z, mean, pre_var)
    S = e.sum(axis=3)
    A = _lse(S, axis=2)
    D = _lse(e, axis=2)
    logp = (-0.5 * (LOG_2PI + z * z)).sum(axis=2)
    diag = S[:, np.arange(B), np.arange(B)]
    return dict(mi=diag - A + c, tc=A - D.sum(axis=2) + (L - 1) * c, dwkl=D.sum(axis=2) - L * c - logp,
                dwkl_dim=D - c + 0.5 * (LOG_2PI + z * z), A=A, D=D, S=S, p=np.exp(S - A[:, :, None]), diag=diag, logp=logp)


def backward(z, mean, pre_var, coef):
    """coef [K, B, 3]: the gradients that reached (mi, tc, dwkl) -> (dz [K, B, L], dmean [B, L], dpre_var [B, L]), partial
    derivatives with z, mean and pre_var held independent"""
    z, m, p = np.asarray(z, np.float64), np.asarray(mean, np.float64), np.asarray(pre_var, np.float64)
    coef = np.asarray(coef, np.float64)
    K, B, L = z.shape
    e = ell(z, m, p)
    S = e.sum(axis=3)
    A = _lse(S, axis=2)
    D = _lse(e, axis=2)
    pj = np.exp(S - A[:, :, None])
    r = np.exp(e - D[:, :, None, :])
    a, b, c3 = coef[..., 0], coef[..., 1], coef[..., 2]
    eye = np.eye(B)[None, :, :, None]
    G = a[:, :, None, None] * eye + (b - a)[:, :, None, None] * pj[..., None] + (c3 - b)[:, :, None, None] * r
    iv = np.exp(np.abs(p))[None, None]
    d = z[:, :, None, :] - m[None, None]
    dz = (G * (-d * iv)).sum(axis=2) + c3[:, :, None] * z
    dmean = (G * (d * iv)).sum(axis=(0, 1))
    dlv = (G * (-0.5 + 0.5 * d * d * iv)).sum(axis=(0, 1))
    return dz, dmean, -np.sign(p) * dlv


def accumulate(comps, dwkl_dim, acc=None):
    """comps [K, B, 3], dwkl_dim [K, B, L] -> acc [4 + L] with the count and the sums added (a new array)"""
    comps, dd = np.asarray(comps, np.float64), np.asarray(dwkl_dim, np.float64)
    L = dd.shape[2]
    acc = np.zeros(ROWS + L) if acc is None else np.array(acc, np.float64)
    acc[0] += comps.shape[0] * comps.shape[1]
    acc[1:4] += comps.reshape(-1, 3).sum(axis=0)
    acc[4:] += dd.reshape(-1, L).sum(axis=0)
    return acc


def finish(acc):
    """-> (mi, tc, dwkl, dwkl_dims [L]): the means over the draws accumulated (zeros when there are none)"""
    acc = np.asarray(acc, np.float64)
    n = acc[0] if acc[0] > 0 else 1.0
    return acc[1] / n, acc[2] / n, acc[3] / n, acc[4:] / n


def rsample(mean, pre_var, eps):
    """z [K, B, L] = mean + exp(lv / 2) eps"""
    m, p, eps = np.asarray(mean, np.float64), np.asarray(pre_var, np.float64), np.asarray(eps, np.float64)
    return m[None] + np.exp(-0.5 * np.abs(p))[None] * eps


def tcvae_term(mean, pre_var, eps, w, alpha, beta, gamma, c):
    """The latent part of the beta-TCVAE loss, (1/B) sum_i w_i (1/K) sum_k (alpha mi + beta tc + gamma dwkl) with
    z = rsample(mean, pre_var, eps), and its TOTAL gradient by mean and pre_var (the backward above, then the rsample chain)
    -> (term, dmean [B, L], dpre_var [B, L], forward dict)"""
    m, p, eps = np.asarray(mean, np.float64), np.asarray(pre_var, np.float64), np.asarray(eps, np.float64)
    K, B, L = eps.shape
    ww = np.ones(B) if w is None else np.asarray(w, np.float64)
    z = rsample(m, p, eps)
    f = forward(z, m, p, c)
    cw = ww[None, :] / (B * K)
    term = (cw * (alpha * f["mi"] + beta * f["tc"] + gamma * f["dwkl"])).sum()
    coef = np.stack([alpha * cw, beta * cw, gamma * cw], axis=-1) * np.ones((K, 1, 1))
    dz, dm, dp = backward(z, m, p, coef)
    sd = np.exp(-0.5 * np.abs(p))
    dm = dm + dz.sum(axis=0)
    # z = mean + exp(-|p| / 2) eps:  dz/dp = -sign(p) / 2 * exp(-|p| / 2) eps
    dp = dp + (dz * eps).sum(axis=0) * sd * (-0.5 * np.sign(p))
    return term, dm, dp, f
