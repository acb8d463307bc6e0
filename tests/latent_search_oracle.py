"""CPU restatement (numpy, float32 or float64) of the guided latent search of csrc/latent_search.hip, from its contract in
include/ggpm_hip.h: the objective J = prop + anchor_weight anchor + prior_weight prior, gradient descent with heavy-ball
momentum, the delta exit, and the choice of the best start.  The heads are property_oracle's (lists of (W [out, in], b [out]),
the last one Linear(w, 1)); the mixture term is latent_prior_oracle's, fp64 in both runs and rounded where the kernel rounds
(its gradient once, to the run's dtype, before it is weighed; its value once, where it is stored).

``Margins`` records the smallest relative margin of every decision and the decisions themselves, so that two runs can be
compared decision by decision:
  * a ReLU sign: |pre| / (sum_k |W_jk x_k| + |b_j|) -- the pre-activation against the magnitude of its summands, which is
    what the rounding error of the dot product scales with;
  * the exit test prop <= delta: |prop - delta| / max(|prop|, |delta|);
  * the selection: (second-smallest J - smallest J) / max of their magnitudes, per molecule with K > 1."""
import numpy as np

import latent_prior_oracle as lpo
from property_oracle import head_backward, head_forward

LOG_2PI = lpo.LOG_2PI


class Margins:
    def __init__(self):
        self.min = np.inf
        self.by_kind = {}                   # "relu" / "delta" / "select" -> that kind's smallest margin
        self.decisions = []

    def add(self, kind, m, taken):
        if np.size(m):
            self.by_kind[kind] = min(self.by_kind.get(kind, np.inf), float(np.min(m)))
            self.min = min(self.min, self.by_kind[kind])
        self.decisions.append(np.asarray(taken).reshape(-1).astype(np.int64))

    def same_decisions(self, other):
        return len(self.decisions) == len(other.decisions) and all(
            a.shape == b.shape and (a == b).all() for a, b in zip(self.decisions, other.decisions))


def _rel(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.nan_to_num(d, nan=np.inf)


def _cast(layers, dt):
    return [(np.asarray(W).astype(dt), np.asarray(b).astype(dt)) for W, b in layers]


def _heads(heads, v, half, margins):
    """both heads on one row v [L] -> ([o_h, o_l], [acts_h, acts_l])"""
    outs, acts = [], []
    for hi, layers in enumerate(heads):
        o, a = head_forward(layers, v[None, hi * half:(hi + 1) * half])
        if margins is not None:
            for i, (W, b) in enumerate(layers[:-1]):
                x = a[i].astype(np.float64)
                W64, b64 = W.astype(np.float64), b.astype(np.float64)
                pre, scale = x @ W64.T + b64, np.abs(x) @ np.abs(W64).T + np.abs(b64)
                margins.add("relu", np.abs(pre) / np.maximum(scale, 1e-300), a[i + 1] > 0)
        outs.append(o[0])
        acts.append(a)
    return outs, acts


def _prop(o, t, w):
    dh, dl = o[0] - t[0], o[1] - t[1]
    return w[0] * (dh * dh) + w[1] * (dl * dl)


def mixture_neg_logp(v, prior):
    """-log p(v) under prior = (logits, means, log_vars), fp64 from the values given -> float64"""
    return -float(lpo.forward(np.asarray(v, np.float64)[None], *prior)["logp"][0])


def mixture_neg_logp_grad(v, prior):
    """d(-log p)/dv = sum_c gamma_c (v - m_c) exp(-s_c), fp64 -> float64 [L]"""
    return -lpo.backward(np.asarray(v, np.float64)[None], *prior, np.ones(1), True)[0][0]


def terms(heads, v, half, mu, iv, t, w, prior, dt, margins=None):
    """(o [2], (prop, anchor, prior)) at v: prop in the run's dtype; anchor and prior summed in fp64 from the dtype's v, mu and
    exp(-lv), rounded once"""
    o, _ = _heads(heads, v, half, margins)
    v64 = v.astype(np.float64)
    d = v64 - mu.astype(np.float64)
    anchor = dt(0.5 * (d * d * iv.astype(np.float64)).sum())
    pr = dt(0.5 * (LOG_2PI + v64 * v64).sum()) if prior is None else dt(mixture_neg_logp(v64, prior))
    return o, (_prop(o, t, w), anchor, pr)


def objective(homo, lumo, v, half, mu, lv, t_h, t_l, w_h, w_l, anchor_weight, prior_weight, prior=None):
    """J(v) in fp64 with its gradient as the search forms it -> (J, dJ/dv [L])"""
    dt = np.float64
    heads = (_cast(homo, dt), _cast(lumo, dt))
    v, mu, iv = np.asarray(v, dt), np.asarray(mu, dt), np.exp(-np.asarray(lv, dt))
    t, w = (dt(t_h), dt(t_l)), (dt(w_h), dt(w_l))
    o, (prop, anchor, pr) = terms(heads, v, half, mu, iv, t, w, prior, dt)
    return prop + anchor_weight * anchor + prior_weight * pr, gradient(heads, v, half, mu, iv, t, w, dt(anchor_weight),
                                                                       dt(prior_weight), prior, dt)[0]


def gradient(heads, v, half, mu, iv, t, w, aw, pw, prior, dt, margins=None):
    """-> (dJ/dv in the run's dtype, prop): a term whose weight is exactly 0 is not evaluated"""
    o, acts = _heads(heads, v, half, margins)
    g = np.empty_like(v)
    for hi in range(2):
        gout = (dt(2) * w[hi]) * (o[hi] - t[hi])
        g[hi * half:(hi + 1) * half] = head_backward(heads[hi], acts[hi], np.asarray([gout], dtype=dt))[0][0]
    if aw != 0:
        g = g + aw * ((v - mu) * iv)
    if pw != 0:
        g = g + pw * (v if prior is None else mixture_neg_logp_grad(v, prior).astype(dt))
    return g, _prop(o, t, w)


def select(J, K, B):
    """the start with the smallest J per molecule: ties to the lowest k, a NaN behind every number, all NaN -> 0"""
    J = np.asarray(J).reshape(K, B)
    best = np.zeros(B, np.int64)
    for b in range(B):
        jb = J[0, b]
        for k in range(1, K):
            j = J[k, b]
            if not np.isnan(j) and (np.isnan(jb) or j < jb):
                best[b], jb = k, j
    return best


def search(homo, lumo, z0, half, mu, lv, t_h, t_l, K, B, lr, momentum, steps, delta, w_h=1.0, w_l=1.0, anchor_weight=0.0,
           prior_weight=0.0, prior=None, dtype=np.float64, margins=None, trace=None):
    """The contract of ggpm_latent_search_guided and ggpm_latent_search_select on z0 [K B, ld] -> dict(z [R, ld], pred [2, R],
    terms [R, 3], J [R], steps [R], best [B]).  ``trace``: a list that receives J before every update of row 0."""
    dt = np.dtype(dtype).type
    heads = (_cast(homo, dt), _cast(lumo, dt))
    z = np.array(z0, dtype=dt)
    R, L = K * B, 2 * half
    assert z.shape[0] == R
    mu = np.asarray(mu, dtype=dt)
    iv = np.exp(-np.asarray(lv, dtype=dt))                     # the kernel's expf(-lv)
    th, tl = np.asarray(t_h, dtype=dt), np.asarray(t_l, dtype=dt)
    lr, momentum, delta = dt(lr), dt(momentum), dt(delta)
    w, aw, pw = (dt(w_h), dt(w_l)), dt(anchor_weight), dt(prior_weight)
    if prior is not None:
        prior = tuple(np.asarray(p, np.float32).astype(np.float64) for p in prior)
    pred, out_terms = np.zeros((2, R), dt), np.zeros((R, 3), dt)
    J, n_steps = np.zeros(R, dt), np.zeros(R, np.int64)
    for r in range(R):
        b = r % B
        v, m, t = z[r, :L].copy(), np.zeros(L, dt), (th[b], tl[b])
        for _ in range(steps):
            g, prop = gradient(heads, v, half, mu[b], iv[b], t, w, aw, pw, prior, dt, margins)
            if trace is not None and r == 0:
                trace.append(float(np.dot(np.array(terms(heads, v, half, mu[b], iv[b], t, w, prior, dt)[1], np.float64),
                                           [1.0, float(aw), float(pw)])))
            if delta >= 0:
                if margins is not None:
                    margins.add("delta", _rel(prop, delta), prop <= delta)
                if prop <= delta:
                    break
            m = momentum * m + g
            v = v - lr * m
            n_steps[r] += 1
        o, tm = terms(heads, v, half, mu[b], iv[b], t, w, prior, dt, margins)
        z[r, :L] = v
        pred[:, r], out_terms[r] = o, tm
        J[r] = (tm[0] + aw * tm[1]) + pw * tm[2]
    best = select(J, K, B)
    if margins is not None and K > 1:
        Jk = np.sort(np.asarray(J, np.float64).reshape(K, B), axis=0)
        margins.add("select", _rel(Jk[0], Jk[1]), best)
    return dict(z=z, pred=pred, terms=out_terms, J=J, steps=n_steps, best=best)
