"""The mixture-of-Gaussians prior restated in numpy fp64 from DESIGN.md (*A learned prior*): the forward (log-density, its
difference to the standard normal's, responsibilities), the backward and the sampler's component choice on the seeded stream
of tests/sample_oracle.py.  Inputs are widened exactly; nothing here is fp32.  CPU only."""
import numpy as np

import sample_oracle as S

SITE_PRIOR_COMP = 260       # include/ggpm_hip.h GGPM_SITE_SAMPLE_PRIOR_COMP
LOG_2PI = float(np.log(2.0 * np.pi))


def _f64(*xs):
    return [np.asarray(x, np.float64) for x in xs]


def logsumexp(x, axis):
    m = x.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def log_pi(a):
    (a,) = _f64(a)
    return a - logsumexp(a, 0)


def forward(z, a, m, s):
    """z [R, L], a [C], m, s [C, L] -> dict(comp [R, C], logp [R], logn [R], ratio [R], resp [R, C])"""
    z, a, m, s = _f64(z, a, m, s)
    d = z[:, None, :] - m[None]
    comp = log_pi(a)[None] - 0.5 * (LOG_2PI + s[None] + d * d * np.exp(-s)[None]).sum(axis=2)
    logp = logsumexp(comp, 1)
    logn = -0.5 * (LOG_2PI + z * z).sum(axis=1)
    return dict(comp=comp, logp=logp, logn=logn, ratio=logp - logn, resp=np.exp(comp - logp[:, None]))


def backward(z, a, m, s, g, on_logp):
    """the gradient of sum_r g[r] ratio[r] (on_logp: logp[r]) -> (dz [R, L], dm [C, L], ds [C, L], da [C])"""
    z, a, m, s, g = _f64(z, a, m, s, g)
    f = forward(z, a, m, s)
    gam, iv = f["resp"], np.exp(-s)
    d = z[:, None, :] - m[None]                                             # [R, C, L]
    w = g[:, None] * gam                                                    # [R, C]
    dz = g[:, None] * ((gam[:, :, None] * (-d * iv[None])).sum(axis=1) + (0.0 if on_logp else 1.0) * z)
    dm = (w[:, :, None] * (d * iv[None])).sum(axis=0)
    ds = (w[:, :, None] * (0.5 * (d * d * iv[None] - 1.0))).sum(axis=0)
    da = (g[:, None] * (gam - np.exp(log_pi(a))[None])).sum(axis=0)
    return dz, dm, ds, da


def uniforms(seed, ids):
    """u = m(PRIOR_COMP, id, 0, 0) 2^-24 -> fp64 [rows]"""
    return S.words(seed, SITE_PRIOR_COMP, ids, 0, 0).astype(np.float64) * 2.0 ** -24


def choose(a, u):
    """the smallest c whose prefix sum of exp(a - max a), taken in index order, exceeds u * total; the last component with a
    non-zero weight if none does -> (components int64 [rows], the distance of u * total from the nearest prefix sum, as a
    fraction of total)"""
    (a,) = _f64(a)
    e = np.exp(a - a.max())
    pre = np.cumsum(e)                                                      # sequential, index order
    total = pre[-1]
    t = np.asarray(u, np.float64) * total
    over = pre[None, :] > t[:, None]
    last = int(np.nonzero(e > 0)[0][-1])
    comp = np.where(over.any(axis=1), over.argmax(axis=1), last)
    return comp.astype(np.int64), np.abs(pre[None, :] - t[:, None]).min(axis=1) / total


def components(seed, ids, a):
    return choose(a, uniforms(seed, ids))


def sample(seed, ids, a, m, s):
    """-> (out fp64 [rows, L] = m_c + exp(s_c / 2) n with the fp64 normals of sample_oracle, components)"""
    a, m, s = _f64(a, m, s)
    comp, _ = components(seed, ids, a)
    n = S.normals(seed, ids, m.shape[1])
    return m[comp] + np.exp(0.5 * s[comp]) * n, comp
