"""numpy restatements for ``log_likelihood`` (*Per-molecule ELBO and the importance-weighted bound*): the draw
key of the latent normals on the stream of tests/sample_oracle.py, and fp64 forms of the three kernels of
csrc/mol_loss.hip.  CPU only."""
import numpy as np

import sample_oracle as SO

SITE_LATENT = 259       # include/ggpm_hip.h GGPM_SITE_SAMPLE_LATENT
MAX_K = 1024            # GGPM_LIKELIHOOD_MAX_K


def latent_normals(seed, ids, K, L, dtype=np.float64):
    """eps[k, b, c]: Box-Muller of m(LATENT, ids[b], k * L + c, 0 / 1) -> [K, B, L]"""
    ids = np.asarray(ids).reshape(1, -1, 1)
    ctr = (np.arange(K).reshape(-1, 1, 1) * L + np.arange(L).reshape(1, 1, -1))
    m0, m1 = SO.words(seed, SITE_LATENT, ids, ctr, 0), SO.words(seed, SITE_LATENT, ids, ctr, 1)
    u1 = ((m0 + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    u2 = (m1.astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1)).astype(dtype)
    return (r * np.cos(dtype(np.pi) * (dtype(2.0) * u2))).astype(dtype)


def mol_parts(terms, B):
    """terms: four (row_loss, mol) or None -> parts [B, 4] in fp64; rows of molecules outside [0, B) count nowhere"""
    parts = np.zeros((B, 4), np.float64)
    for t, term in enumerate(terms):
        if term is None:
            continue
        v, mol = np.asarray(term[0], np.float64), np.asarray(term[1])
        keep = (mol >= 0) & (mol < B)
        np.add.at(parts[:, t], mol[keep], v[keep])
    return parts


def latent_terms(mean, pre_var, eps):
    """fp64: -> (z [K, B, L], kl [B], logpq [K, B])"""
    m, e = np.asarray(mean, np.float64), np.asarray(eps, np.float64)
    lv = -np.abs(np.asarray(pre_var, np.float64))
    z = m[None] + np.exp(lv / 2)[None] * e
    kl = -0.5 * (1.0 + lv - m * m - np.exp(lv)).sum(axis=1)
    logpq = -0.5 * (z * z).sum(axis=2) + 0.5 * (e * e + lv[None]).sum(axis=2)
    return z, kl, logpq


def iwae_finish(parts, logpq, kl):
    """fp64: -> (elbo [B], iwae [B]), the logsumexp over k with its maximum subtracted"""
    nll = np.asarray(parts, np.float64).sum(axis=2)
    w = np.asarray(logpq, np.float64) - nll
    mx = w.max(axis=0)
    iwae = mx + np.log(np.exp(w - mx[None]).sum(axis=0)) - np.log(len(w))
    return -nll.mean(axis=0) - np.asarray(kl, np.float64), iwae
