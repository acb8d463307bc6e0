"""numpy fp64 restatement of the four operations ``bound_loss`` adds (include/ggpm_hip.h, *Training on the bound*): the
objective with its coefficients, the row scaling by molecule, the per-molecule weight of the tree-only attachment head's
backward, and the backward of the latent terms.  tests/test_mol_objective_cpu.py checks the gradient formulas here against
central differences of the forward functions here; the GPU tests compare the kernels with these."""
import numpy as np


def nll_of(parts):
    p = np.asarray(parts, np.float64)
    return (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def objective(parts, logpq, kl, w, objective, beta):
    """-> (loss, c_nll [K, B], c_logpq [K, B], c_kl [B])"""
    nll, logpq, kl = nll_of(parts), np.asarray(logpq, np.float64), np.asarray(kl, np.float64)
    K, B = nll.shape
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    if objective == "elbo":
        loss = (w * (nll.mean(axis=0) + beta * kl)).sum() / B
        return loss, np.broadcast_to(w / (K * B), (K, B)).copy(), np.zeros((K, B)), beta * w / B
    if beta != 1.0:
        raise ValueError("the importance-weighted bound has no beta")
    lw = logpq - nll
    mx = lw.max(axis=0)
    e = np.exp(lw - mx[None])
    se = e.sum(axis=0)
    iwae = mx + np.log(se) - np.log(K)
    c = w[None] * (e / se[None]) / B
    return -(w * iwae).sum() / B, c, -c, np.zeros(B)


def scale_rows_by_mol(d, N, mol, coef, B, g=1.0):
    """-> d with d[m, :N] *= g * coef[mol[m]] (0 where the molecule is outside [0, B)); columns past N are left alone"""
    d = np.array(d, np.float64)
    d2 = d.reshape(d.shape[0], -1)
    mol = np.asarray(mol)
    ok = (mol >= 0) & (mol < B)
    s = np.where(ok, g * np.asarray(coef, np.float64)[np.where(ok, mol, 0)], 0.0)
    d2[:, :N] = np.where(ok[:, None], d2[:, :N] * s[:, None], 0.0)
    return d2.reshape(d.shape)


def latent_terms(mean, pre_var, eps):
    """-> (z [K, B, L], kl [B], logpq [K, B])"""
    m, p, e = (np.asarray(a, np.float64) for a in (mean, pre_var, eps))
    lv = -np.abs(p)
    z = m[None] + np.exp(lv / 2)[None] * e
    kl = -0.5 * (1.0 + lv - m * m - np.exp(lv)).sum(axis=1)
    logpq = -0.5 * (z * z).sum(axis=2) + 0.5 * (e * e + lv[None]).sum(axis=2)
    return z, kl, logpq


def latent_terms_backward(dz, mean, pre_var, eps, c_logpq, c_kl, g=1.0):
    """-> (dmean [B, L], dpre_var [B, L]) of  sum(dz * z) + g sum(c_logpq * logpq) + g sum(c_kl * kl)"""
    m, p, e = (np.asarray(a, np.float64) for a in (mean, pre_var, eps))
    K, B, L = e.shape
    dz = np.zeros((K, B, L)) if dz is None else np.asarray(dz, np.float64)
    G = g * (np.zeros((K, B)) if c_logpq is None else np.asarray(c_logpq, np.float64))
    gk = g * (np.zeros(B) if c_kl is None else np.asarray(c_kl, np.float64))
    lv = -np.abs(p)
    sd = np.exp(lv / 2)
    z = m[None] + sd[None] * e
    a = dz - G[:, :, None] * z
    dmean = a.sum(axis=0) + gk[:, None] * m
    dlv = (a * (0.5 * sd[None] * e) + 0.5 * G[:, :, None]).sum(axis=0) - 0.5 * gk[:, None] * (1.0 - np.exp(lv))
    return dmean, -np.sign(p) * dlv


def assm_weight(meta, coef, B, g=1.0):
    """The upstream gradient of every attachment prediction in ggpm_motif_assm_backward_weighted: g * coef[molecule]"""
    mol = np.asarray(meta)[:, 3]
    ok = (mol >= 0) & (mol < B)
    return np.where(ok, g * np.asarray(coef, np.float64)[np.where(ok, mol, 0)], 0.0)
