"""GPU: the two entries the STL / DReG estimators add (csrc/mol_loss.hip: ggpm_iwae_weights, ggpm_latent_terms_backward_path)
called on their own against the fp64 numpy forms of tests/mol_estimator_oracle.py.  One wave owns one output and its lanes
stride the samples, so the shapes go past 64 and past 128 samples (lane striding, the shuffle tree), through 1, 3 and 65
molecules and 1, 8 and 65 latent columns; pre_var has both signs, exact zeros and magnitudes up to 30, where the fp32
sd = expf(lv / 2) is about 3e-7 and r = exp(-lv / 2) about 3e6.

Bounds, with u = 2^-24 (half an fp32 ulp, relative) and fp64(K) = (K + 16) 2^-52:
  * weights: fp32 inputs are exact, everything is formed in fp64 and rounded once -> u |s| + fp64(K) max(|lw|, 1) |s| (2^-150,
    half the smallest subnormal, where a weight underflows fp32), as the coefficients of ggpm_bound_objective; ess adds the
    squares of the unrounded weights (each twice the weights' relative error, K + 2 more roundings) -> u |ess| + 3 fp64(K)
    max(|lw|, 1) |ess|.
  * path backward: sd and z are re-formed in fp32 like the forward, sd within 2u (expf) and z within
    z_err = u (3 |sd eps| + |z|); r, G = g c_logpq, t = dz - G z, a = t + G eps r and every product and sum are fp64.  With
    q = s (1 without) and se = |sd eps|:
        dmean: sum_k |q| |G| z_err                          + fp64(K) sum_k |q| (|dz| + |G z| + |G eps r|) + u |dmean|
        dlv:   sum_k |q| (|G| z_err se / 2 + |t| u se)      + fp64(K) sum_k |q| (|t| se + |G| eps^2) / 2    + u |dlv|
    (|t| u se is the 2u of sd in t sd eps / 2; G eps^2 / 2 is written multiplied out and carries fp64 roundings only).
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure.  The measured maxima are printed as
fractions of the bounds."""
import numpy as np
import pytest
import torch

import mol_estimator_oracle as E
import mol_objective_oracle as O
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT = -777.25
ERR_ARG = 1
P = F_._p
SLACK = 1.0 + 2.0 ** -10


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------- ggpm_iwae_weights
def weights_case(K, B):
    rs = np.random.RandomState(K * 100 + B + 7)
    parts = (rs.rand(K, B, 4) * 2).astype(np.float32)
    if K > 1:
        parts[:, :, 0] += np.linspace(20.0, 140.0, K).astype(np.float32)[rs.permutation(K)][:, None]    # nll spread 120 over k
    parts[:, B // 2, 3] = 0.0
    logpq = (rs.standard_normal((K, B)) * 3).astype(np.float32)
    logpq[:, 0] += 200.0
    return parts, logpq


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 130])
def test_weights_and_ess_equal_fp64(K, B):
    parts, logpq = weights_case(K, B)
    got = F_.iwae_weights(dev(parts), dev(logpq))
    s, ess = (f64(t) for t in got)
    s64, ess64 = E.iwae_weights(parts, logpq)
    lw = logpq.astype(np.float64) - O.nll_of(parts)
    fp64 = (K + 16) * 2.0 ** -52 * max(np.abs(lw).max(), 1.0)
    bs = (U * SLACK + fp64) * s64 + 2.0 ** -150
    be = (U * SLACK + 3 * fp64) * ess64
    es, ee = np.abs(s - s64), np.abs(ess - ess64)
    print("K %d B %d: s %.3e (%.2f of its bound), ess %.3e (%.2f)" % (K, B, es.max(), (es / bs).max(), ee.max(), (ee / be).max()))
    assert (es <= bs).all() and (ee <= be).all()
    assert bs.max() <= 1e-4 * s64.max() and be.max() <= 1e-4 * ess64.max()
    assert (np.abs(s.sum(axis=0) - 1.0) <= K * (U * SLACK + fp64)).all()                      # a softmax
    assert (ess >= 1.0).all() and (ess <= K).all() and np.isfinite(s).all()
    if K == 1:
        assert (s == 1.0).all() and (ess == 1.0).all()
    again = F_.iwae_weights(dev(parts), dev(logpq))
    assert all(torch.equal(a, b) for a, b in zip(got, again))                                 # run to run


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 130])
def test_weights_identities(K, B):
    parts, logpq = weights_case(K, B)
    # equal log-weights: exp(0) = 1, a sum of K ones, one division, one rounding
    eq_parts, eq_logpq = np.broadcast_to(parts[:1], parts.shape).copy(), np.broadcast_to(logpq[:1], logpq.shape).copy()
    s, ess = F_.iwae_weights(dev(eq_parts), dev(eq_logpq))
    assert (f64(s) == float(np.float32(1.0 / K))).all() and (f64(ess) == float(K)).all()
    # one sample 200 nats ahead of the others, at another k in every molecule
    lead = (np.arange(B) * 7) % K
    far = logpq.copy()
    lw = far.astype(np.float64) - O.nll_of(parts)
    far[lead, np.arange(B)] += np.float32(200.0) + (lw.max(axis=0) - lw[lead, np.arange(B)]).astype(np.float32)
    s, ess = F_.iwae_weights(dev(parts), dev(far))
    want = np.zeros((K, B))
    want[lead, np.arange(B)] = 1.0
    assert np.array_equal(f64(s), want) and (f64(ess) == 1.0).all()


@pytest.mark.parametrize("K", [1, 3, 64, 65, 130])
def test_one_unweighted_molecule_has_the_objectives_coefficients(K):
    parts, logpq = weights_case(K, 1)
    s, _ = F_.iwae_weights(dev(parts), dev(logpq))
    kl = torch.zeros(1, device=DEV)
    _, c_nll, _, _ = F_.bound_objective(dev(parts), dev(logpq), kl, None, "iwae", 1.0)
    assert torch.equal(s, c_nll)
    # with ess absent the weights are the same
    s2 = torch.empty_like(s)
    assert _lib.load().ggpm_iwae_weights(P(dev(parts)), P(dev(logpq)), K, 1, P(s2), None, F_._stream()) == 0
    assert torch.equal(s, s2)


# ---------------------------------------------------------------------------------------------- ggpm_latent_terms_backward_path
PV_PATTERN = (0.8, -1.3, 0.0, 30.0, 1e-4, -30.0, -0.4, 12.0, -1e-4, 2.5, -7.0)


def path_case(K, B, L):
    rs = np.random.RandomState(K * 10000 + B * 100 + L + 3)
    mean = rs.standard_normal((B, L)).astype(np.float32)
    pv = (np.resize(np.asarray(PV_PATTERN), B * L) * (1 + 0.1 * rs.rand(B * L))).astype(np.float32).reshape(B, L)
    eps = rs.standard_normal((K, B, L)).astype(np.float32)
    dz = rs.standard_normal((K, B, L)).astype(np.float32)
    s = rs.dirichlet(np.ones(K) * 0.7, size=B).T.astype(np.float32)                       # [K, B], columns sum to 1
    c_pq = (-(rs.rand(B) + 0.2)[None] * s / B).astype(np.float32)                        # -w s / B
    return mean, pv, eps, dz, c_pq, s


def path_bounds(dz, mean, pv, eps, c_pq, s, g):
    """-> (bound of dmean, bound of dlv), both [B, L], from the docstring's formulas"""
    K, B, L = eps.shape
    m, e = mean.astype(np.float64), eps.astype(np.float64)
    lv = -np.abs(pv.astype(np.float64))
    sd = np.exp(lv / 2)[None]
    with np.errstate(over="ignore"):
        r = np.exp(-lv / 2)[None]
    z = m[None] + sd * e
    se = np.abs(sd * e)
    z_err = U * (3 * se + np.abs(z))
    G = g * (np.zeros((K, B)) if c_pq is None else c_pq.astype(np.float64))[:, :, None]
    q = np.abs(np.ones((K, B, 1)) if s is None else s.astype(np.float64)[:, :, None])
    d = np.zeros((K, B, L)) if dz is None else dz.astype(np.float64)
    t = np.abs(d - G * z)
    G = np.abs(G)
    with np.errstate(invalid="ignore"):
        Ger = np.where(G * np.abs(e) != 0.0, G * np.abs(e) * r, 0.0)
    fp64 = (K + 16) * 2.0 ** -52
    dm, dp = E.latent_terms_backward_path(dz, mean, pv, eps, c_pq, s, g)
    bm = (q * G * z_err).sum(axis=0) + fp64 * (q * (np.abs(d) + G * np.abs(z) + Ger)).sum(axis=0) + U * np.abs(dm)
    bp = (q * (G * z_err * se / 2 + t * U * se)).sum(axis=0) + fp64 * (q * (t * se + G * e * e) / 2).sum(axis=0) + U * np.abs(dp)
    return dm, dp, bm * SLACK, bp * SLACK


VARIANTS = [("stl", False, True, False), ("dreg g", True, True, True), ("dreg no dz", True, False, False),
            ("stl no dz g", False, False, True)]


@pytest.mark.parametrize("L", [1, 8, 65])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("K", [1, 3, 65, 130])
def test_path_backward_equals_fp64_within_the_derived_bounds(K, B, L):
    mean, pv, eps, dz, c_pq, s = path_case(K, B, L)
    if B * L >= len(PV_PATTERN):
        assert (pv > 0).any() and (pv < 0).any() and (pv == 0).any() and np.abs(pv).max() >= 30
    for what, with_s, with_dz, with_g in VARIANTS:
        a_dz, a_s = dz if with_dz else None, s if with_s else None
        g = np.float32(0.6) if with_g else None
        args = (dev(a_dz), dev(mean), dev(pv), dev(eps), dev(c_pq), dev(a_s), dev(np.array([g])) if with_g else None)
        dmean, dpv = (f64(t) for t in F_.latent_terms_backward_path(*args))
        dm64, dp64, bm, bp = path_bounds(a_dz, mean, pv, eps, c_pq, a_s, float(g) if with_g else 1.0)
        em, ep = np.abs(dmean - dm64), np.abs(dpv - dp64)
        print("K %d B %d L %d %s: dmean %.3e (%.2f of its bound), dpre_var %.3e (%.2f)"
              % (K, B, L, what, em.max(), (em / bm).max(), ep.max(), (ep / np.maximum(bp, 1e-300)).max()))
        assert (em <= bm).all(), float((em / bm).max())
        assert (ep <= bp).all(), float((ep / np.maximum(bp, 1e-300)).max())
        assert (dpv[pv == 0] == 0).all()                                 # d(-|p|)/dp = 0 at 0
        assert np.isfinite(dmean).all() and np.isfinite(dpv).all()
        assert bm.max() <= 1e-4 * np.abs(dm64).max() and (bp.max() <= 1e-4 * np.abs(dp64).max() or not dp64.any())
        again = F_.latent_terms_backward_path(*args)
        assert np.array_equal(f64(again[0]), dmean) and np.array_equal(f64(again[1]), dpv)          # run to run


@pytest.mark.parametrize("K,B,L", [(1, 3, 8), (3, 3, 8), (65, 3, 65), (130, 65, 8)])
def test_exact_properties(K, B, L):
    mean, pv, eps, dz, c_pq, s = path_case(K, B, L)
    run = lambda *a: F_.latent_terms_backward_path(*[dev(x) for x in a])
    # s of ones is no s
    plain = run(dz, mean, pv, eps, c_pq, None)
    ones = run(dz, mean, pv, eps, c_pq, np.ones((K, B), np.float32))
    assert torch.equal(plain[0], ones[0]) and torch.equal(plain[1], ones[1])
    if K == 1:                                                           # one sample: its weight is 1.0f, DReG is STL
        s1, _ = F_.iwae_weights(torch.zeros(1, B, 4, device=DEV), dev(c_pq))
        assert bool((s1 == 1.0).all())
        got = F_.latent_terms_backward_path(dev(dz), dev(mean), dev(pv), dev(eps), dev(c_pq), s1)
        assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    # eps = 0: no path term and z = mean -- dmean is the reparameterised kernel's
    zero = np.zeros_like(eps)
    a = run(dz, mean, pv, zero, c_pq, None)
    b = F_.latent_terms_backward(dev(dz), dev(mean), dev(pv), dev(zero), dev(c_pq), None)
    assert torch.equal(a[0], b[0]) and not bool(a[1].ne(0).any())
    # a decoder gradient that cancels the rest: G z - G eps r, rounded to fp32 -- what is left is rounding
    for with_s in (False, True):
        q = s if with_s else None
        G = c_pq.astype(np.float64)[:, :, None]
        lv = -np.abs(pv.astype(np.float64))
        z = mean.astype(np.float64)[None] + np.exp(lv / 2)[None] * eps.astype(np.float64)
        cancel = (G * z - G * eps.astype(np.float64) * np.exp(-lv / 2)[None]).astype(np.float32)
        dmean, dpv = (f64(t) for t in run(cancel, mean, pv, eps, c_pq, q))
        dm64, dp64, bm, bp = path_bounds(cancel, mean, pv, eps, c_pq, q, 1.0)
        qq = np.ones((K, B, 1)) if q is None else q.astype(np.float64)[:, :, None]
        rm = (qq * U * np.abs(cancel)).sum(axis=0)                      # the rounding of dz itself, which the reference keeps
        rp = (qq * U * np.abs(cancel) * np.abs(np.exp(lv / 2)[None] * eps) / 2).sum(axis=0)
        assert (np.abs(dm64) <= rm * SLACK).all() and (np.abs(dp64) <= (rp + bp) * SLACK).all()
        print("K %d B %d L %d s %d: cancelling dz leaves dmean %.3e of %.3e, dpre_var %.3e"
              % (K, B, L, with_s, np.abs(dmean).max(), np.abs(cancel).max(), np.abs(dpv).max()))
        assert (np.abs(dmean - dm64) <= bm).all() and (np.abs(dpv - dp64) <= bp).all()
        assert (np.abs(dmean) <= bm + rm * SLACK).all() and (np.abs(dpv) <= bp + (rp + bp) * SLACK).all()


def test_a_molecule_without_weight_gets_finite_zeros_where_the_reciprocal_overflows():
    K, B, L = 65, 3, 8
    mean, pv, eps, dz, c_pq, s = path_case(K, B, L)
    pv[1] = np.float32(3e38) * np.where(np.arange(L) % 2 == 0, 1, -1).astype(np.float32)
    c_pq[:, 1] = 0.0
    c_pq[::2, 1] = -0.0
    dz[:, 1] = 0.0
    for q in (None, s):
        dmean, dpv = (f64(t) for t in F_.latent_terms_backward_path(dev(dz), dev(mean), dev(pv), dev(eps), dev(c_pq), dev(q)))
        assert np.isfinite(dmean).all() and np.isfinite(dpv).all()
        assert not dmean[1].any() and not dpv[1].any()
        assert dmean[0].any() and dmean[2].any()


# ---------------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_are_refused_before_any_launch():
    lib, st = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    iw = lambda **kw: lib.ggpm_iwae_weights(*[kw.get(k, v) for k, v in (
        ("parts", P(f)), ("logpq", P(f)), ("K", 2), ("B", 3), ("s", P(f)), ("ess", P(f)))], st)
    assert iw(K=0) == ERR_ARG and iw(K=1025) == ERR_ARG and iw(B=0) == ERR_ARG and iw(B=-1) == ERR_ARG
    assert iw(parts=None) == ERR_ARG and iw(logpq=None) == ERR_ARG and iw(s=None) == ERR_ARG
    bw = lambda **kw: lib.ggpm_latent_terms_backward_path(*[kw.get(k, v) for k, v in (
        ("dz", P(f)), ("mean", P(f)), ("pre_var", P(f)), ("eps", P(f)), ("c_logpq", P(f)), ("s", P(f)), ("g", None), ("K", 2),
        ("B", 3), ("L", 8), ("dmean", P(f)), ("dpre_var", P(f)))], st)
    assert bw(K=0) == ERR_ARG and bw(K=1025) == ERR_ARG and bw(B=0) == ERR_ARG and bw(L=0) == ERR_ARG
    assert bw(mean=None) == ERR_ARG and bw(pre_var=None) == ERR_ARG and bw(eps=None) == ERR_ARG
    assert bw(dmean=None) == ERR_ARG and bw(dpre_var=None) == ERR_ARG
    assert bw(B=1 << 20, L=1 << 11) == ERR_ARG                                                        # B * L = 2^31
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all()                                                            # nothing ran
