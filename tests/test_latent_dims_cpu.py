"""CPU: the numpy oracle of the per-dimension entries (tests/latent_dims_oracle.py) against central differences of its own
loss, against tests/mol_objective_oracle.py at lambda = 0, and against numpy.var; plus the host-side argument checks of
``bound_loss(free_bits=...)`` that need no GPU."""
import numpy as np
import pytest

import latent_dims_oracle as D
import mol_objective_oracle as O


def _inputs(K, B, L, seed):
    rs = np.random.RandomState(seed)
    mean = rs.standard_normal((B, L))
    pv = rs.standard_normal((B, L)) * 1.5
    nll = np.abs(rs.standard_normal((K, B))) * 7
    w = np.abs(rs.standard_normal(B)) + 0.25
    return mean, pv, nll, w


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


def _lambdas(kb):
    """0, a midpoint between two neighbouring klbar_j, and a value above all of them"""
    s = np.sort(kb)
    mid = 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) > 1 else 0.5 * s[0]
    return [0.0, float(mid), float(s[-1] * 1.5 + 1.0)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,B,L", [(1, 1, 3), (2, 3, 8), (3, 5, 4)])
def test_free_bits_gradient_is_the_central_difference_of_the_loss(K, B, L, weighted):
    mean, pv, nll, w = _inputs(K, B, L, 100 * B + L)
    w = w if weighted else None
    beta = 0.3
    kb = D.klbar(mean, pv, w)
    for lam in _lambdas(kb):
        assert (np.abs(kb - lam) >= 1e-3 * np.maximum(np.abs(kb), lam)).all()         # no column within 1e-3 relative of lambda
        assert (np.abs(pv) > 1e-3).all()                                               # |.| is differentiable at every point
        f = lambda: D.free_bits_loss(nll, mean, pv, w, beta, lam)
        dm, dp = D.free_bits_kl_backward(mean, pv, w, lam, g=beta)
        assert np.abs(_central(f, mean) - dm).max() < 1e-7
        assert np.abs(_central(f, pv) - dp).max() < 1e-7
        if lam > kb.max():
            assert not dm.any() and not dp.any()
            assert abs(D.free_bits_kl(mean, pv, w, lam)[1] - L * lam) <= 4 * np.finfo(float).eps * L * lam


@pytest.mark.parametrize("weighted", [False, True])
def test_lambda_zero_is_the_elbos_kl(weighted):
    K, B, L = 2, 4, 6
    mean, pv, nll, w = _inputs(K, B, L, 5)
    w = w if weighted else None
    beta = 0.3
    eps = np.zeros((K, B, L))
    parts = np.zeros((K, B, 4))
    parts[:, :, 0] = nll
    _, kl, logpq = O.latent_terms(mean, pv, eps)
    loss, _, _, c_kl = O.objective(parts, logpq, kl, w, "elbo", beta)
    loss0 = O.objective(parts, logpq, kl, w, "elbo", 0.0)[0]
    assert (D.klbar(mean, pv, w) > 0).all()
    got = D.free_bits_loss(nll, mean, pv, w, beta, 0.0)
    assert abs(got - loss) <= 1e-14 * abs(loss)
    assert abs(beta * D.free_bits_kl(mean, pv, w, 0.0)[1] - (loss - loss0)) <= 1e-13 * abs(loss)
    # the gradient of the KL part: the c_kl route of the latent backward
    dm, dp = D.free_bits_kl_backward(mean, pv, w, 0.0, g=beta)
    wm, wp = O.latent_terms_backward(None, mean, pv, eps, None, c_kl)
    assert np.abs(dm - wm).max() <= 1e-15 * np.abs(wm).max() and np.abs(dp - wp).max() <= 1e-15 * np.abs(wp).max()
    # kl_dim sums to the per-molecule kl
    assert np.abs(D.kl_dim(mean, pv).sum(axis=1) - kl).max() <= 1e-14 * np.abs(kl).max()


def test_a_column_exactly_at_lambda_is_free():
    mean, pv, _, _ = _inputs(1, 4, 3, 9)
    kb = D.klbar(mean, pv)
    dm, dp = D.free_bits_kl_backward(mean, pv, None, kb[1])
    assert not dm[:, 1].any() and not dp[:, 1].any()
    assert dm[:, kb > kb[1]].any() or not (kb > kb[1]).any()
    z = np.zeros((2, 3))
    assert not D.kl_dim(z, z).any()                                                   # mean = 0, pre_var = 0: exactly 0
    dm, dp = D.free_bits_kl_backward(np.ones((2, 3)), z, None, 0.0)
    assert not dp.any()                                                                # sign(0) = 0


def test_accumulator_statistics_are_numpys():
    rs = np.random.RandomState(3)
    mean = rs.standard_normal((300, 5))
    mean[:, 2] = 100.0 + 0.01 * rs.standard_normal(300)
    pv = rs.standard_normal((300, 5))
    acc = D.accumulate(mean, pv)
    out, n_active = D.finish(acc, 0.01)
    assert np.abs(out[2] - np.var(mean, axis=0)).max() <= 1e-9                        # (the cancelling column: 1e4 * 300 * 2^-52)
    assert np.abs(out[2][[0, 1, 3, 4]] - np.var(mean, axis=0)[[0, 1, 3, 4]]).max() <= 1e-14
    assert np.abs(out[1] - mean.mean(axis=0)).max() <= 1e-13
    assert np.abs(out[3] - np.exp(-np.abs(pv)).mean(axis=0)).max() <= 1e-15
    assert np.abs(out[0] - D.klbar(mean, pv)).max() <= 1e-12
    assert np.array_equal(out[4], out[2] + out[3])
    assert n_active == 4 and D.finish(acc, 0.0)[1] == 5 and D.finish(acc, 10.0)[1] == 0
    # batch by batch is the whole
    parts = D.accumulate(mean[65:], pv[65:], D.accumulate(mean[1:65], pv[1:65], D.accumulate(mean[:1], pv[:1])))
    assert np.abs(parts - acc).max() <= 1e-15 * 300 * np.abs(acc).max()
    # nothing accumulated: zeros, nothing active
    out0, n0 = D.finish(np.zeros((5, 4)), 0.01)
    assert not out0.any() and n0 == 0


def test_the_binding_declares_the_four_entries():
    from ggpm_amd import _lib, build
    for name in ("ggpm_latent_dim_accumulate", "ggpm_latent_dim_finish", "ggpm_free_bits_kl", "ggpm_free_bits_kl_backward"):
        assert name in _lib.SIGNATURES
    assert "latent_dims.hip" in build.SOURCES
    from ggpm_amd import functional as F_
    import re
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ggpm_hip.h")).read()
    assert int(re.search(r"#define GGPM_FREE_BITS_MAX_L (\d+)", text).group(1)) == F_.FREE_BITS_MAX_L
    assert int(re.search(r"#define GGPM_LATENT_STAT_ROWS (\d+)", text).group(1)) == F_.LATENT_STAT_ROWS == D.ROWS
    assert int(re.search(r"#define GGPM_LATENT_STAT_OUT (\d+)", text).group(1)) == F_.LATENT_STAT_ROWS


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from ggpm_amd import functional as F_
    m = torch.zeros(3, 4)
    with pytest.raises(RuntimeError):
        F_.free_bits_kl(m, m, None, 0.1)
    with pytest.raises(RuntimeError):
        F_.latent_dim_accumulate(m, m, torch.zeros(5, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        F_.latent_dim_finish(torch.zeros(5, 4, dtype=torch.float64))


def test_free_bits_keyword_is_on_both_forms_of_bound_loss():
    import inspect
    from ggpm_amd import property_vae as PV
    for fn in (PV.bound_loss, PV._VAE.bound_loss):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "free_bits" and inspect.signature(fn).parameters["free_bits"].default is None
    info = PV.FreeBitsObjective(1, 2, 3, 4, 5, 6, {"a": 1}, kl_dims="k", free_bits=0.5)
    assert isinstance(info, PV.MolObjective) and len(info) == 7 and tuple(info)[:6] == (1, 2, 3, 4, 5, 6)
    assert info.kl_dims == "k" and info.free_bits == 0.5 and info.stats == {"a": 1}
    assert PV.LatentStats._fields == ("kl_dims", "mu_mean", "mu_var", "sigma2_mean", "agg_var", "n_active", "n_molecules")
