"""CPU: the numpy oracle of the ``bound_loss`` operations (tests/mol_objective_oracle.py) against central differences of its
own forward, and against the reference's loss in every fixture of tests/golden/make_golden_mol_objective.py."""
import numpy as np
import pytest

import mol_objective_fixtures as OF
import mol_objective_oracle as O

RS = np.random.RandomState(7)


def _inputs(K, B, spread=1.0):
    parts = np.abs(RS.standard_normal((K, B, 4))) * 5
    logpq = RS.standard_normal((K, B)) * spread
    kl = np.abs(RS.standard_normal(B)) * 3
    w = np.abs(RS.standard_normal(B)) + 0.25
    return parts, logpq, kl, w


def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        old = x[i]
        x[i] = old + h
        up = f()
        x[i] = old - h
        dn = f()
        x[i] = old
        g[i] = (up - dn) / (2 * h)
    return g


@pytest.mark.parametrize("objective,beta,weighted", [("elbo", 0.3, True), ("elbo", 1.0, False), ("iwae", 1.0, True),
                                                     ("iwae", 1.0, False)])
@pytest.mark.parametrize("K,B", [(1, 1), (3, 3), (5, 2)])
def test_objective_coefficients_are_the_partial_derivatives(objective, beta, weighted, K, B):
    parts, logpq, kl, w = _inputs(K, B)
    w = w if weighted else None
    loss, c_nll, c_logpq, c_kl = O.objective(parts, logpq, kl, w, objective, beta)
    f = lambda: O.objective(parts, logpq, kl, w, objective, beta)[0]
    d_parts = _central(f, parts)
    for t in range(4):                              # nll is the plain sum of the four terms
        assert np.abs(d_parts[:, :, t] - c_nll).max() < 1e-7
    assert np.abs(_central(f, logpq) - c_logpq).max() < 1e-7
    assert np.abs(_central(f, kl) - c_kl).max() < 1e-7
    if objective == "iwae":
        s = c_nll * B / (np.ones(B) if w is None else w)[None]
        assert np.abs(s.sum(axis=0) - 1).max() < 1e-14


def test_softmax_survives_log_weights_more_than_100_apart():
    parts, logpq, kl, w = _inputs(4, 2)
    logpq[0] += 400.0
    logpq[2] -= 300.0
    loss, c_nll, _, _ = O.objective(parts, logpq, kl, None, "iwae", 1.0)
    assert np.isfinite(loss) and np.isfinite(c_nll).all()
    assert np.abs(c_nll.sum(axis=0) * 2 - 1).max() < 1e-14


def test_iwae_with_beta_raises():
    parts, logpq, kl, w = _inputs(2, 2)
    with pytest.raises(ValueError):
        O.objective(parts, logpq, kl, None, "iwae", 0.5)


@pytest.mark.parametrize("K,B,L", [(1, 1, 3), (3, 2, 4)])
def test_latent_terms_backward_is_the_gradient_of_latent_terms(K, B, L):
    mean, pv, eps = RS.standard_normal((B, L)), RS.standard_normal((B, L)), RS.standard_normal((K, B, L))
    assert (pv > 0).any() and (pv < 0).any()
    dz, c_pq, c_kl, g = RS.standard_normal((K, B, L)), RS.standard_normal((K, B)), RS.standard_normal(B), 0.7

    def f():
        z, kl, logpq = O.latent_terms(mean, pv, eps)
        return (dz * z).sum() + g * (c_pq * logpq).sum() + g * (c_kl * kl).sum()

    dmean, dpv = O.latent_terms_backward(dz, mean, pv, eps, c_pq, c_kl, g)
    assert np.abs(_central(f, mean) - dmean).max() < 1e-7
    assert np.abs(_central(f, pv) - dpv).max() < 1e-7
    # pre_var == 0: d(-|p|)/dp = 0, ggpm_rsample_backward's convention
    pv0 = pv.copy()
    pv0[0, 0] = 0.0
    assert O.latent_terms_backward(dz, mean, pv0, eps, c_pq, c_kl, g)[1][0, 0] == 0.0


def test_scale_rows_by_mol_oracle():
    d = RS.standard_normal((5, 6))
    mol = np.array([0, 2, -1, 3, 1])
    coef = np.array([2.0, 3.0, 5.0])
    out = O.scale_rows_by_mol(d, 4, mol, coef, 3, g=0.5)
    assert np.array_equal(out[:, 4:], d[:, 4:])
    assert np.allclose(out[0, :4], d[0, :4] * 1.0) and np.allclose(out[1, :4], d[1, :4] * 2.5) and np.allclose(out[4, :4], d[4, :4] * 1.5)
    assert (out[2, :4] == 0).all() and (out[3, :4] == 0).all()
    meta = np.array([[2, 1, 0, 1, 0, 0], [1, 2, 3, 7, 2, 2]])
    assert np.array_equal(O.assm_weight(meta, coef, 3, g=2.0), [6.0, 0.0])


@pytest.mark.parametrize("name", OF.names())
def test_oracle_objective_is_the_references_loss(name):
    g = OF.ObjGolden(name)
    z = g.z
    loss = O.objective(z["parts"], z["logpq"], z["kl"], g.weights, g.objective, g.beta)[0]
    ref = float(z["loss"])
    print("%s: oracle %.9g reference %.9g" % (name, loss, ref))
    assert abs(loss - ref) <= 1e-5 * abs(ref)
    # one file per case and variant, data only, each smaller than the largest fixture committed before (1.3 MB)
    import os
    assert os.path.getsize(os.path.join(OF.GOLDEN_DIR, name + ".npz")) < 1_000_000
    assert set(g.grads(32)) == set(g.grads(64)) and len(g.grads(32)) > 10


def test_every_case_has_every_variant():
    import mol_likelihood_fixtures as LF
    assert OF.names() == sorted("%s__%s" % (c, v) for c in LF.names() for v in OF.VARIANTS)
