"""CPU: the numpy oracle of the STL / DReG estimators (tests/mol_estimator_oracle.py) against torch fp64 autograd of the
surrogate loss that defines them, for unbiasedness on a one-dimensional toy model (DReG minus the reparameterised gradient has
zero mean; STL minus it has not), and at the true posterior, where the path gradient vanishes sample by sample; plus the host
side of ``bound_loss(estimator=...)`` that needs no GPU.

The surrogate, with s the normalised importance weights held constant:
    lw_k = -0.5 |z_k|^2 + 0.5 sum_j ((z_k - mean.detach())^2 exp(-lv.detach()) + lv.detach()) - nll(z_k)
    loss = -(1/B) sum_i w_i sum_k s_ki.detach() lw_ki
Its gradient is the STL estimator; DReG multiplies what arrives at z_k by s_k once more (a hook on z_k)."""
import numpy as np
import pytest
import torch

import mol_estimator_oracle as E
import mol_objective_oracle as O


def _nll_torch(z, a, v):
    """any smooth nll: [.., B, L] -> [.., B]"""
    return ((z - a) ** 2 * 0.7).sum(dim=-1) + torch.sin((z * v).sum(dim=-1))


@pytest.mark.parametrize("estimator", ["stl", "dreg"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [1, 3])
def test_the_oracle_is_autograd_of_the_surrogate(K, weighted, estimator):
    B, L = 3, 5
    rs = np.random.RandomState(10 * K + weighted)
    mean, pv = rs.standard_normal((B, L)), rs.standard_normal((B, L)) * 1.5
    eps = rs.standard_normal((K, B, L))
    a, v = rs.standard_normal(L), rs.standard_normal(L) * 0.5
    w = np.abs(rs.standard_normal(B)) + 0.25 if weighted else np.ones(B)
    assert (pv > 0).any() and (pv < 0).any()

    tm, tp = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (mean, pv))
    ta, tv, te, tw = (torch.tensor(x, dtype=torch.float64) for x in (a, v, eps, w))
    lv = -tp.abs()
    zs, lws = [], []
    for k in range(K):
        zk = tm + torch.exp(lv / 2) * te[k]
        zs.append(zk)
        lws.append(-0.5 * (zk * zk).sum(dim=-1) + 0.5 * ((zk - tm.detach()) ** 2 * torch.exp(-lv.detach()) + lv.detach()).sum(dim=-1)
                   - _nll_torch(zk, ta, tv))
    lw = torch.stack(lws)
    s = torch.softmax(lw.detach(), dim=0)
    if estimator == "dreg":
        for k in range(K):
            zs[k].register_hook(lambda grad, k=k: grad * s[k][:, None])
    loss = -(tw[None] * s * lw).sum() / B
    loss.backward()

    # what the kernels are given: the decoder's gradient at z (it carries c = w s / B), the coefficient of logpq, and s
    z64, _, logpq = O.latent_terms(mean, pv, eps)
    zt = torch.tensor(z64, dtype=torch.float64, requires_grad=True)
    nll = _nll_torch(zt, ta, tv)
    dnll, = torch.autograd.grad(nll.sum(), zt)
    parts = np.zeros((K, B, 4))
    parts[:, :, 0] = nll.detach().numpy()
    s64, ess = E.iwae_weights(parts, logpq)
    assert np.abs(s64 - s.numpy()).max() <= 1e-14 and (ess >= 1 - 1e-12).all() and (ess <= K + 1e-12).all()
    c = w[None] * s64 / B
    dm, dp = E.latent_terms_backward_path(c[:, :, None] * dnll.numpy(), mean, pv, eps, -c, s64 if estimator == "dreg" else None)
    for got, want in ((dm, tm.grad.numpy()), (dp, tp.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    if K == 1:                                                    # s = 1: the two estimators coincide
        dm1, dp1 = E.latent_terms_backward_path(c[:, :, None] * dnll.numpy(), mean, pv, eps, -c, None)
        assert np.array_equal(dm, dm1) and np.array_equal(dp, dp1) and np.array_equal(s64, np.ones((1, B)))


# ---------------------------------------------------------------------------------------------- the toy model
# one latent, p(z) = N(0, 1), nll(z) = (z - 1.3)^2 / 1.4 (a N(1.3, 0.7) likelihood up to a constant)
def _toy(mean, lv, K, N, eps):
    """Per draw (the N "molecules" share mean and lv, weights B so that no 1/N enters) the three estimators of
    d(-iwae)/d(mean, lv) -> {name: (dmean [N], dlv [N])}"""
    m, p = np.full((N, 1), mean), np.full((N, 1), lv)           # pre_var = lv < 0: dpre_var = dlv
    assert lv < 0
    z, kl, logpq = O.latent_terms(m, p, eps)
    parts = np.zeros((K, N, 4))
    parts[:, :, 0] = ((z - 1.3) ** 2 / 1.4)[:, :, 0]
    s, _ = E.iwae_weights(parts, logpq)
    c = s                                                        # w_i / B = 1
    dz = c[:, :, None] * (2.0 * (z - 1.3) / 1.4)
    out = {"reparam": O.latent_terms_backward(dz, m, p, eps, -c, None),
           "stl": E.latent_terms_backward_path(dz, m, p, eps, -c, None),
           "dreg": E.latent_terms_backward_path(dz, m, p, eps, -c, s)}
    return {k: (a[:, 0], b[:, 0]) for k, (a, b) in out.items()}


TOY = [(0.2, -0.5, 4, 10 ** 6), (0.2, -0.5, 3, 2 * 10 ** 5), (-0.4, -1.5, 8, 2 * 10 ** 5)]


@pytest.mark.parametrize("mean,lv,K,N", TOY)
def test_dreg_is_unbiased_on_the_toy_model_and_stl_is_not(mean, lv, K, N):
    """E[dreg - reparam] = 0: per run and per parameter |mean| <= 5 standard errors (a condition: the chance that one of the
    36 standard-normal statistics passes 5 is 2e-5); the same statistic of stl - reparam on dmean is in the hundreds."""
    worst = 0.0
    for seed in range(6):
        eps = np.random.default_rng(seed).standard_normal((K, N, 1))
        est = _toy(mean, lv, K, N, eps)
        for i, what in enumerate(("dmean", "dlv")):
            d = est["dreg"][i] - est["reparam"][i]
            stat = abs(d.mean()) / (d.std() / np.sqrt(N))
            worst = max(worst, stat)
            assert stat <= 5.0, (seed, what, stat)
        d = est["stl"][0] - est["reparam"][0]
        biased = abs(d.mean()) / (d.std() / np.sqrt(N))
        print("mean %g lv %g K %d N %d seed %d: stl - reparam on dmean %.1f standard errors" % (mean, lv, K, N, seed, biased))
        assert biased > 50.0, (seed, biased)
    print("mean %g lv %g K %d N %d: largest |mean| / standard error of dreg - reparam %.2f" % (mean, lv, K, N, worst))


def test_the_path_gradient_vanishes_at_the_true_posterior():
    prec = 1.0 + 1.0 / 0.7
    mean, lv = (1.3 / 0.7) / prec, -np.log(prec)
    K, N = 4, 1000
    est = _toy(mean, lv, K, N, np.random.default_rng(0).standard_normal((K, N, 1)))
    for name in ("stl", "dreg"):
        assert max(np.abs(est[name][0]).max(), np.abs(est[name][1]).max()) <= 1e-12, name
    assert np.abs(est["reparam"][0]).max() > 1e-2 and np.abs(est["reparam"][1]).max() > 1e-2


def test_a_sample_without_weight_adds_nothing_even_where_the_reciprocal_overflows():
    K, B, L = 3, 2, 4
    rs = np.random.RandomState(0)
    mean, eps, dz = rs.standard_normal((B, L)), rs.standard_normal((K, B, L)), rs.standard_normal((K, B, L))
    pv = rs.standard_normal((B, L))
    pv[0] = [3e38, -3e38, 3e38, -3e38]
    dz[:, 0] = 0.0
    c = np.abs(rs.standard_normal((K, B)))
    c[:, 0] = 0.0
    dm, dp = E.latent_terms_backward_path(dz, mean, pv, eps, -c, None)
    assert not dm[0].any() and not dp[0].any() and np.isfinite(dm[0]).all()


# ---------------------------------------------------------------------------------------------- the host side
def test_the_binding_declares_the_two_entries():
    from ggpm_amd import _lib
    assert len(_lib.SIGNATURES["ggpm_iwae_weights"][1]) == 7
    assert len(_lib.SIGNATURES["ggpm_latent_terms_backward_path"][1]) == 13


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from ggpm_amd import functional as F_
    K, B, L = 2, 3, 4
    parts, logpq = torch.zeros(K, B, 4), torch.zeros(K, B)
    mean, eps = torch.zeros(B, L), torch.zeros(K, B, L)
    with pytest.raises(RuntimeError):
        F_.iwae_weights(parts, logpq)
    with pytest.raises(RuntimeError):
        F_.latent_terms_backward_path(eps, mean, mean, eps, logpq)
    with pytest.raises(ValueError):
        F_.iwae_weights(parts[:, :, :3], logpq)
    with pytest.raises(ValueError):
        F_.iwae_weights(parts.double(), logpq)
    with pytest.raises(ValueError):
        F_.latent_terms_backward_path(eps, mean[:2], mean, eps, logpq)
    with pytest.raises(ValueError):
        F_.latent_terms_backward_path(eps, mean, mean, eps, logpq, s=torch.zeros(B, K))
    with pytest.raises(ValueError):
        F_.latent_terms_backward_path(eps, mean, mean, eps.double(), logpq)
    with pytest.raises(ValueError):
        F_.latent_terms_backward_path(eps, mean, mean, eps, logpq, g=torch.zeros(2))


def test_estimator_keyword_is_on_both_forms_of_bound_loss():
    import inspect
    from ggpm_amd import property_vae as PV
    for fn in (PV.bound_loss, PV._VAE.bound_loss):
        assert inspect.signature(fn).parameters["estimator"].default == "reparam"
    assert PV.ESTIMATORS == ("reparam", "stl", "dreg")
    info = PV.EstimatorObjective(1, 2, 3, 4, 5, 6, {"a": 1}, estimator="dreg", sample_weights="s", ess="e")
    assert isinstance(info, PV.MolObjective) and len(info) == 7 and tuple(info)[:6] == (1, 2, 3, 4, 5, 6)
    assert (info.estimator, info.sample_weights, info.ess) == ("dreg", "s", "e") and info.stats == {"a": 1}
