"""CPU: the numpy fp64 oracle of the mixture prior (tests/latent_prior_oracle.py) against torch.distributions and fp64 autograd,
its component choice on an exactly representable case, and the host side of ``MixturePrior`` and of the ``prior=`` argument:
what is refused, and refused without a device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import latent_prior_oracle as O
import sample_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E64 = 2.0 ** -52


def _case(R=7, C=5, L=6, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(C)
    m = scale * rs.standard_normal((C, L))
    s = rs.standard_normal((C, L))
    z = rs.standard_normal((R, L)) * 1.5
    g = rs.standard_normal(R)
    return z, a, m, s, g


def _torch_logp(z, a, m, s):
    D = torch.distributions
    mix = D.MixtureSameFamily(D.Categorical(logits=a), D.Independent(D.Normal(m, torch.exp(0.5 * s)), 1))
    return mix.log_prob(z)


@pytest.mark.parametrize("scale", [0.1, 5.0])
def test_oracle_logp_equals_mixture_same_family(scale):
    z, a, m, s, _ = _case(scale=scale)
    f = O.forward(z, a, m, s)
    want = _torch_logp(*[torch.from_numpy(x) for x in (z, a, m, s)]).numpy()
    assert np.abs(f["logp"] - want).max() <= 64 * E64 * np.abs(want).max()
    assert np.abs(f["resp"].sum(axis=1) - 1.0).max() <= 64 * E64
    normal = torch.distributions.Normal(0.0, 1.0).log_prob(torch.from_numpy(z)).sum(dim=1).numpy()
    assert np.abs(f["ratio"] - (want - normal)).max() <= 64 * E64 * (np.abs(want).max() + np.abs(normal).max())


@pytest.mark.parametrize("on_logp", [False, True])
def test_oracle_gradients_equal_fp64_autograd(on_logp):
    z, a, m, s, g = _case()
    g[2] = 0.0
    tz, ta, tm, ts = [torch.from_numpy(x).requires_grad_() for x in (z, a, m, s)]
    out = _torch_logp(tz, ta, tm, ts)
    if not on_logp:
        out = out - torch.distributions.Normal(0.0, 1.0).log_prob(tz).sum(dim=1)
    (out * torch.from_numpy(g)).sum().backward()
    got = O.backward(z, a, m, s, g, on_logp)
    for what, x, t in zip(("dz", "dm", "ds", "da"), got, (tz, tm, ts, ta)):
        w = t.grad.numpy()
        assert np.abs(x - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0), what
    assert not got[0][2].any()


def test_the_standard_prior_has_ratio_zero():
    z = _case(R=9, L=24)[0]
    f = O.forward(z, np.zeros(1), np.zeros((1, 24)), np.zeros((1, 24)))
    assert np.abs(f["ratio"]).max() <= 8 * 24 * E64 * np.abs(f["logn"]).max()
    assert (f["resp"] == 1.0).all()


def test_component_choice_on_two_equal_logits_splits_the_words_exactly_in_half():
    """e = (1, 1), total 2: u = k 2^-24 picks component 1 exactly from k = 2^23 on -- every boundary is representable"""
    a = np.zeros(2)
    n0 = 0
    for lo in range(0, 1 << 24, 1 << 20):
        k = np.arange(lo, lo + (1 << 20))
        comp, _ = O.choose(a, k * 2.0 ** -24)
        assert np.array_equal(comp, (k >= 1 << 23).astype(np.int64))
        n0 += int((comp == 0).sum())
    assert n0 == 1 << 23
    # a zero weight is never drawn, wherever it stands; u = 0 takes the first component with weight
    comp, _ = O.choose(np.array([-1e4, 0.0, -1e4, 0.0, -1e4]), np.array([0.0, 0.25, 0.5, 0.75, 1 - 2.0 ** -24]))
    assert comp.tolist() == [1, 1, 3, 3, 3]
    # the stream's own uniforms: 24-bit, keyed by the id alone
    u = O.uniforms(5, np.arange(64))
    assert np.array_equal(u, O.uniforms(5, np.arange(64)[::-1])[::-1]) and ((u * 2 ** 24) % 1 == 0).all() and len(set(u)) > 60
    assert not np.array_equal(u, O.uniforms(6, np.arange(64)))


def test_header_binding_and_python_constants_agree():
    from ggpm_amd import _lib, functional as F_, prior
    text = open(os.path.join(ROOT, "include", "ggpm_hip.h")).read()
    assert int(re.search(r"#define GGPM_MIXTURE_MAX_C (\d+)", text).group(1)) == F_.MIXTURE_MAX_C >= 256
    site = int(re.search(r"#define GGPM_SITE_SAMPLE_PRIOR_COMP (\d+)", text).group(1))
    assert site == prior.SITE_PRIOR_COMP == O.SITE_PRIOR_COMP
    sites = [int(v) for v in re.findall(r"#define GGPM_SITE_\w+ (\d+)", text)]
    assert len(set(sites)) == len(sites)
    assert len(_lib.SIGNATURES["ggpm_mixture_logp"][1]) == 13
    assert len(_lib.SIGNATURES["ggpm_mixture_logp_backward"][1]) == 16
    assert len(_lib.SIGNATURES["ggpm_sample_mixture"][1]) == 13
    from ggpm_amd import build
    assert "latent_prior.hip" in build.SOURCES
    # the host copy of the stream's words is the oracle's
    ids = np.arange(100)
    assert np.array_equal(prior._stream_words(*S.split(12345678901234), site, ids, 1, 0), S.words(12345678901234, site, ids, 1, 0))


def test_mixture_prior_arguments_and_initialisation():
    from ggpm_amd.prior import MixturePrior
    for bad in (dict(n_components=0, latent_size=4), dict(n_components=4097, latent_size=4), dict(n_components=2, latent_size=0),
                dict(n_components=2, latent_size=4097), dict(n_components=2.0, latent_size=4), dict(n_components=True, latent_size=4),
                dict(n_components=2, latent_size=4, init_std=-1.0), dict(n_components=2, latent_size=4, init_std=float("nan"))):
        with pytest.raises(ValueError):
            MixturePrior(**bad)
    torch.manual_seed(3)
    p = MixturePrior(3, 5, init_std=2.0)
    torch.manual_seed(3)
    q = MixturePrior(3, 5, init_std=2.0)
    assert torch.equal(p.means, q.means) and p.means.std() > 0.5
    assert not p.logits.any() and not p.log_vars.any()
    assert sorted(n for n, _ in p.named_parameters()) == ["log_vars", "logits", "means"]
    assert all(t.dtype == torch.float32 and t.requires_grad for t in p.parameters())
    assert (p.means.shape, p.log_vars.shape, p.logits.shape) == ((3, 5), (3, 5), (3,))
    std = MixturePrior.standard(7)
    assert std.n_components == 1 and std.latent_size == 7 and not std.means.any() and not std.log_vars.any()


def test_mixture_prior_has_no_cpu_path_and_checks_z():
    from ggpm_amd import functional as F_
    from ggpm_amd.prior import MixturePrior
    p = MixturePrior(3, 5)
    z = torch.zeros(4, 5)
    for call in (lambda: p.log_prob(z), lambda: p.log_ratio(z), lambda: p.responsibilities(z), lambda: p.sample(4, seed=1)):
        with pytest.raises(RuntimeError):
            call()
    for bad in (torch.zeros(4, 6), torch.zeros(4, 5, dtype=torch.float64), torch.zeros(0, 5), "z"):
        with pytest.raises(ValueError):
            p.log_ratio(bad)
    with pytest.raises(ValueError):
        p.sample(0, seed=1)
    a, m, s = p.logits.detach(), p.means.detach(), p.log_vars.detach()
    with pytest.raises(RuntimeError):
        F_.mixture_logp(z, a, m, s)
    with pytest.raises(RuntimeError):
        F_.sample_mixture(a, m, s, 4, 1, 2)
    with pytest.raises(ValueError):
        F_.mixture_logp(z, a[:2], m, s)
    with pytest.raises(ValueError):
        F_.mixture_logp(z.double(), a, m, s)
    with pytest.raises(ValueError):
        F_.mixture_logp(z, a, m, s[:, :4])
    with pytest.raises(ValueError):
        F_.sample_mixture(a, m, s, 4, 1, 2, ids=[0, 1, 2])
    with pytest.raises(ValueError):
        F_.mixture_logp_backward(z, a, m, s, torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                                 torch.zeros(3), False)
    with pytest.raises(ValueError):
        F_.mixture_logp_backward(z, a, m, s, torch.zeros(4, 3), torch.zeros(4, dtype=torch.float64), torch.zeros(4), False)


def test_init_from_latents_takes_rows_by_the_seeded_stream():
    from ggpm_amd.prior import MixturePrior, SITE_PRIOR_COMP
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.standard_normal((50, 4)) * np.array([1.0, 2.0, 0.5, 3.0])).to(torch.float32)
    p = MixturePrior(3, 4).init_from_latents(x, seed=9)
    rows = np.argsort(S.words(9, SITE_PRIOR_COMP, np.arange(50), 1, 0), kind="stable")[:3]
    assert torch.equal(p.means.detach(), x[torch.from_numpy(rows)]) and len(set(rows.tolist())) == 3
    want = torch.log(x.double().var(dim=0, unbiased=False)).to(torch.float32)
    assert torch.equal(p.log_vars.detach(), want.expand(3, 4)) and not p.logits.any()
    q = MixturePrior(3, 4).init_from_latents(x, seed=9)
    assert torch.equal(p.means, q.means)
    assert not torch.equal(MixturePrior(3, 4).init_from_latents(x, seed=10).means, p.means)
    with pytest.raises(ValueError):
        MixturePrior(3, 4).init_from_latents(x[:2], seed=9)
    with pytest.raises(ValueError):
        MixturePrior(3, 4).init_from_latents(x[:, :3], seed=9)


def test_prior_keyword_and_its_refusals_need_no_device():
    from ggpm_amd import objectives as OB, property_vae as PV
    from ggpm_amd.prior import MixturePrior, check_prior
    for fn in (PV.bound_loss, PV._VAE.bound_loss, PV.log_likelihood, PV._VAE.log_likelihood, PV._VAE.sample, PV._sample):
        assert inspect.signature(fn).parameters["prior"].default is None
    p = MixturePrior(3, 8)
    cpu = torch.device("cpu")
    assert check_prior("m.bound_loss", None, 8, cpu) is None and check_prior("m.bound_loss", p, 8, cpu) is p
    with pytest.raises(ValueError, match="8 latent columns"):
        check_prior("m.bound_loss", p, 24, cpu)
    with pytest.raises(ValueError, match="MixturePrior"):
        check_prior("m.bound_loss", torch.nn.Linear(2, 2), 8, cpu)
    with pytest.raises(ValueError, match="the prior is on"):
        check_prior("m.bound_loss", p, 8, torch.device("meta"))
    args = dict(name="m", B=4, L=8, beta=1.0, alpha=None, gamma=None)
    with pytest.raises(ValueError, match="standard normal"):
        OB.VARIANTS["free_bits"](objective="elbo", dataset_size=None, free_bits=0.5, prior=p, **args)
    with pytest.raises(ValueError, match="standard normal"):
        OB.VARIANTS["tcvae"](objective="tcvae", dataset_size=1000, free_bits=None, prior=p, **args)
    for key, objective in (("plain", "elbo"), ("plain", "iwae"), ("stl", "iwae"), ("dreg", "iwae")):
        OB.VARIANTS[key](objective=objective, dataset_size=None, free_bits=None, prior=p, **args)
    # the result types: the leading fields stay, the two attributes are added
    info = PV.PriorObjective(1, 2, 3, 4, 5, 6, {"a": 1}, log_prior_ratio="r", kl_standard="k")
    assert isinstance(info, PV.MolObjective) and tuple(info) == (1, 2, 3, 4, 5, 6, {"a": 1})
    assert (info.log_prior_ratio, info.kl_standard) == ("r", "k")
    est = PV.PriorEstimatorObjective(1, 2, 3, 4, 5, 6, {}, estimator="stl", sample_weights="s", ess="e", log_prior_ratio="r",
                                     kl_standard="k")
    assert isinstance(est, PV.EstimatorObjective) and (est.estimator, est.ess, est.kl_standard) == ("stl", "e", "k")
    ll = PV.PriorLikelihood(1, 2, 3, 4, 5, {}, log_prior_ratio="r", kl_standard="k")
    assert isinstance(ll, PV.MolLikelihood) and len(ll) == 6 and ll.kl == 2 and ll.log_prior_ratio == "r"
