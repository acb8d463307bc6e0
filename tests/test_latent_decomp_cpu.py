"""CPU: the fp64 restatement of the KL split (tests/latent_decomp_oracle.py) against torch autograd in fp64, the identities
the split obeys, the constants the binding shares with the header, and the argument errors that need no device."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import latent_decomp_oracle as O


def _inputs(K, B, L, seed):
    rs = np.random.RandomState(seed)
    mean = rs.standard_normal((B, L)) * 0.7
    pv = rs.standard_normal((B, L)) * 1.2
    eps = rs.standard_normal((K, B, L))
    coef = rs.standard_normal((K, B, 3))
    return mean, pv, eps, coef


def _torch_parts(z, mean, pv, c):
    """(mi, tc, dwkl) [K, B] in torch fp64 ops, written from the definitions (not from the oracle's code)"""
    K, B, L = z.shape
    lv = -pv.abs()
    e = -0.5 * (math.log(2 * math.pi) + lv[None, None] + (z[:, :, None, :] - mean[None, None]) ** 2 * torch.exp(-lv)[None, None])
    S = e.sum(dim=3)
    A = torch.logsumexp(S, dim=2)
    D = torch.logsumexp(e, dim=2)
    logp = (-0.5 * (math.log(2 * math.pi) + z * z)).sum(dim=2)
    diag = S[:, torch.arange(B), torch.arange(B)]
    return diag - A + c, A - D.sum(dim=2) + (L - 1) * c, D.sum(dim=2) - L * c - logp


@pytest.mark.parametrize("K,B,L", [(1, 1, 1), (2, 3, 4), (3, 7, 5)])
def test_backward_is_torch_autograds_in_fp64(K, B, L):
    mean, pv, eps, coef = _inputs(K, B, L, 10 * B + L)
    z = O.rsample(mean, pv, eps)
    c = O.log_nb(1000, B)
    tz, tm, tp = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (z, mean, pv))
    mi, tc, dwkl = _torch_parts(tz, tm, tp, c)
    f = O.forward(z, mean, pv, c)
    for a, b in ((mi, f["mi"]), (tc, f["tc"]), (dwkl, f["dwkl"])):
        assert np.abs(a.detach().numpy() - b).max() <= 1e-12 * (1 + np.abs(b).max())
    tcoef = torch.tensor(coef)
    (tcoef[..., 0] * mi + tcoef[..., 1] * tc + tcoef[..., 2] * dwkl).sum().backward()
    dz, dm, dp = O.backward(z, mean, pv, coef)
    for got, want in ((dz, tz.grad), (dm, tm.grad), (dp, tp.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max())


@pytest.mark.parametrize("weighted", [False, True])
def test_chained_gradient_is_torch_autograds_through_the_rsample(weighted):
    K, B, L = 3, 5, 4
    mean, pv, eps, _ = _inputs(K, B, L, 3)
    w = np.linspace(0.5, 2.0, B) if weighted else None
    c = O.log_nb(777, B)
    term, dm, dp, _ = O.tcvae_term(mean, pv, eps, w, 0.7, 4.0, 1.3, c)
    tm, tp = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mean, pv))
    tz = tm[None] + torch.exp(-0.5 * tp.abs())[None] * torch.tensor(eps)
    mi, tc, dwkl = _torch_parts(tz, tm, tp, c)
    ww = torch.ones(B, dtype=torch.float64) if w is None else torch.tensor(w)
    t = ((0.7 * mi + 4.0 * tc + 1.3 * dwkl) * ww[None, :]).sum() / (B * K)
    t.backward()
    assert abs(float(t.detach()) - term) <= 1e-12 * abs(term)
    assert np.abs(dm - tm.grad.numpy()).max() <= 1e-12 * np.abs(dm).max()
    assert np.abs(dp - tp.grad.numpy()).max() <= 1e-12 * np.abs(dp).max()


def test_the_three_parts_add_up_to_log_q_minus_log_p_whatever_n_is():
    K, B, L = 2, 6, 5
    mean, pv, eps, _ = _inputs(K, B, L, 4)
    z = O.rsample(mean, pv, eps)
    lv = -np.abs(pv)
    logq = (-0.5 * (O.LOG_2PI + lv[None] + eps * eps)).sum(axis=2)          # (z - mean)^2 exp(-lv) = eps^2
    logp = (-0.5 * (O.LOG_2PI + z * z)).sum(axis=2)
    sums = []
    for N in (B, 1000, 10 ** 9):
        f = O.forward(z, mean, pv, O.log_nb(N, B))
        s = f["mi"] + f["tc"] + f["dwkl"]
        scale = np.abs(f["tc"]).max() + np.abs(f["dwkl"]).max() + np.abs(f["mi"]).max()
        assert np.abs(s - (logq - logp)).max() <= 1e-13 * scale
        assert np.abs(f["dwkl_dim"].sum(axis=2) - f["dwkl"]).max() <= 1e-13 * scale
        sums.append(s)
    assert np.abs(sums[0] - sums[2]).max() <= 1e-12 * np.abs(sums[0]).max()


def test_one_molecule_gives_log_n_and_no_total_correlation_beyond_the_constant():
    """B = 1: S = A and sum_l D = S, so mi = c = log N and tc = (L - 1) c exactly -- the constant minibatch-weighted sampling
    leaves when the batch is the whole estimate of q(z); it is 0 for one latent column and for N = 1.  (With the formulas as
    they stand tc is NOT 0 for B = 1, L > 1, N > 1: log q(z) and every log q_l(z_l) each carry their own -c.)"""
    K, B = 3, 1
    for L, N in ((6, 12345), (1, 12345), (6, 1)):
        mean, pv, eps, _ = _inputs(K, B, L, 5)
        z = O.rsample(mean, pv, eps)
        f = O.forward(z, mean, pv, O.log_nb(N, B))
        assert np.abs(f["mi"] - math.log(N)).max() <= 1e-13 * max(math.log(N), 1.0)
        assert np.abs(f["tc"] - (L - 1) * math.log(N)).max() <= 1e-12 * max(L * math.log(N), 1.0)
        if L == 1 or N == 1:
            assert np.abs(f["tc"]).max() <= 1e-12
        assert (f["p"] == 1.0).all()


def test_accumulator_and_finish():
    rs = np.random.RandomState(6)
    c1, d1 = rs.standard_normal((2, 5, 3)), rs.standard_normal((2, 5, 4))
    c2, d2 = rs.standard_normal((2, 3, 3)), rs.standard_normal((2, 3, 4))
    acc = O.accumulate(c2, d2, O.accumulate(c1, d1))
    assert acc.shape == (O.ROWS + 4,) and acc[0] == 16
    mi, tc, dwkl, dims = O.finish(acc)
    allc = np.concatenate([c1.reshape(-1, 3), c2.reshape(-1, 3)])
    assert np.allclose([mi, tc, dwkl], allc.mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(dims, np.concatenate([d1.reshape(-1, 4), d2.reshape(-1, 4)]).mean(axis=0), rtol=1e-13, atol=0)
    assert O.finish(np.zeros(O.ROWS + 4))[:3] == (0.0, 0.0, 0.0)


def test_the_binding_declares_the_three_entries_and_the_headers_constants():
    from ggpm_amd import _lib, build
    from ggpm_amd import functional as F_
    for name in ("ggpm_latent_decomp", "ggpm_latent_decomp_backward", "ggpm_latent_decomp_accumulate"):
        assert name in _lib.SIGNATURES
    assert "latent_decomp.hip" in build.SOURCES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ggpm_hip.h")).read()
    assert int(re.search(r"#define GGPM_LATENT_DECOMP_ROWS (\d+)", text).group(1)) == F_.LATENT_DECOMP_ROWS == O.ROWS
    assert int(re.search(r"#define GGPM_LATENT_DECOMP_MAX_B (\d+)", text).group(1)) == F_.LATENT_DECOMP_MAX_B
    assert "tcvae" not in F_.BOUND_OBJECTIVES


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from ggpm_amd import functional as F_
    z, m = torch.zeros(2, 3, 4), torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.latent_decomposition(z, m, m, 10)
    lj, ld, coef = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.latent_decomposition_backward(z, m, m, lj, ld, coef)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.latent_decomp_accumulate(coef, z, torch.zeros(8, dtype=torch.float64))
    for bad in (lambda: F_.latent_decomposition(z, m, m, 2),                                   # dataset_size < B
                lambda: F_.latent_decomposition(z, m, m, 10.0),
                lambda: F_.latent_decomposition(z, m, m, True),
                lambda: F_.latent_decomposition(z, m[:2], m, 10),
                lambda: F_.latent_decomposition(z[0], m, m, 10),
                lambda: F_.latent_decomposition(z.double(), m, m, 10),
                lambda: F_.latent_decomposition(torch.zeros(F_.LIKELIHOOD_MAX_K + 1, 1, 1), m[:1, :1], m[:1, :1], 10),
                lambda: F_.latent_decomposition_backward(z, m, m, lj, ld, coef[:, :, :2]),
                lambda: F_.latent_decomposition_backward(z, m, m, lj.float(), ld, coef),
                lambda: F_.latent_decomposition_backward(z, m, m, lj, ld[:, :, :3], coef),
                lambda: F_.latent_decomposition_backward(z, m, m, lj, ld, coef.double()),
                lambda: F_.latent_decomp_accumulate(coef, z, torch.zeros(9, dtype=torch.float64)),
                lambda: F_.latent_decomp_accumulate(coef, z, torch.zeros(8)),
                lambda: F_.latent_decomp_accumulate(coef[:1], z, torch.zeros(8, dtype=torch.float64))):
        with pytest.raises(ValueError):
            bad()


def test_the_new_keywords_are_on_both_forms_of_bound_loss_with_their_defaults():
    from ggpm_amd import property_vae as PV
    for fn in (PV.bound_loss, PV._VAE.bound_loss):
        par = inspect.signature(fn).parameters
        assert list(par)[-4:] == ["alpha", "gamma", "dataset_size", "free_bits"]
        assert all(par[k].default is None for k in ("alpha", "gamma", "dataset_size"))
        assert par["objective"].default == "elbo" and par["beta"].default == 1.0 and par["estimator"].default == "reparam"
    for name in ("latent_decomposition", "latent_decomposition_accumulator"):
        assert list(inspect.signature(getattr(PV._VAE, name)).parameters)[-3:] == ["dataset_size", "n_samples", "seed"]
    assert PV.LatentDecomposition._fields == ("mi", "tc", "dwkl", "dwkl_dims", "kl", "n_molecules")
    assert issubclass(PV.DecompositionObjective, PV.MolObjective)
