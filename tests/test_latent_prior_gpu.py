"""GPU: ``prior=`` of ``log_likelihood``, ``bound_loss`` and ``sample`` end to end on one hierarchical and one tree-only model
(the fixtures of tests/mol_likelihood_fixtures.py and, for ``sample``, the models of tests/test_sampled_decode_gpu.py), and a
post-hoc fit of a ``MixturePrior`` on fixed latents.

The comparison target of the gradients is a fp64 torch restatement of the latent chain with the decoder treated as given: the
call's own ``parts``, the posterior (mean, pre_var) and the draws eps enter as data, and the decoder's dependence on z_k enters
through J[k, i] = d nll[k, i] / d z[k, i], taken from the run (the gradient that arrives at z_k from ``molecule_losses``,
divided by the objective's coefficient of nll[k, i]).  Under autograd in fp64 that gives the gradients of mean and pre_var --
turned into those of ``R_mean`` / ``R_var`` with the encoder's root vectors -- and of the prior's three tensors."""
import functools

import numpy as np
import pytest
import torch

import latent_prior_oracle as O
import mol_likelihood_fixtures as LF
from golden_utils import assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4           # the project's relative parity figure (BASELINE.json)
SEED = 0x1234ABCD5678EF01
TWO = [("ll_hier_gru_s40", "hier-prop"), ("ll_motif_gru_s60", "prop")]
LOG_2PI = O.LOG_2PI


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    g = LF.LLGolden(case)
    batch, sch = g.batch()
    return g, g.model(kind).to(DEV), batch, sch


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _weights(g, weighted):
    return [float(v) for v in np.linspace(0.5, 2.0, g.B)] if weighted else None


def _prior(g, C=3, seed=5):
    from ggpm_amd.prior import MixturePrior
    torch.manual_seed(seed)
    p = MixturePrior(C, g.latent, init_std=0.7)
    with torch.no_grad():
        p.logits.copy_(torch.randn(C) * 0.5)
        p.log_vars.copy_(torch.randn(C, g.latent) * 0.4)
    return p.to(DEV)


def _grads(*modules):
    torch.cuda.synchronize()
    return [{k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None} for m in modules]


def _step(model, prior, **kw):
    """zero_grad, bound_loss, backward -> (loss, info, the model's gradients, the prior's, the decoder's dz per draw)"""
    g, _, batch, sch = kw.pop("case")
    model.zero_grad(set_to_none=True)
    if prior is not None:
        prior.zero_grad(set_to_none=True)
        kw["prior"] = prior
    arrived = {}
    inner = model.decoder.molecule_losses

    def recording(mols, vecs, *a, **k):
        if vecs[0].requires_grad:
            vecs[0].register_hook(lambda grad, n=len(arrived): arrived.__setitem__(n, grad.detach().clone()))
            arrived[len(arrived)] = None
        return inner(mols, vecs, *a, **k)

    model.decoder.molecule_losses = recording
    try:
        loss, info = model.bound_loss(batch, seed=SEED, schedule=sch, **kw)
    finally:
        del model.decoder.molecule_losses
    loss.backward()
    gm, gp = _grads(model, prior) if prior is not None else (_grads(model)[0], {})
    model.zero_grad(set_to_none=True)
    return loss.detach().clone(), info, gm, gp, [arrived[k] for k in sorted(arrived)]


# ---------------------------------------------------------------------------------------------- prior=None and the standard prior
@pytest.mark.parametrize("case,kind", TWO)
def test_prior_none_is_the_call_without_the_argument(case, kind):
    from ggpm_amd.property_vae import MolLikelihood, MolObjective
    c = _case(case, kind)
    g, model, batch, sch = c
    a = model.log_likelihood(batch, n_samples=2, seed=SEED, schedule=sch)
    b = model.log_likelihood(batch, n_samples=2, seed=SEED, schedule=sch, prior=None)
    assert type(a) is type(b) is MolLikelihood and a.stats == b.stats and "prior_launches" not in b.stats
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    for kw in (dict(n_samples=2, objective="elbo", beta=0.3, mol_weights=_weights(g, True)), dict(n_samples=2, objective="iwae"),
               dict(n_samples=2, objective="iwae", estimator="dreg")):
        la, ia, ga, _, _ = _step(model, None, case=c, **kw)
        model.zero_grad(set_to_none=True)
        loss, ib = model.bound_loss(batch, seed=SEED, schedule=sch, prior=None, **kw)
        loss.backward()
        gb = _grads(model)[0]
        model.zero_grad(set_to_none=True)
        assert torch.equal(la, loss.detach()) and type(ia) is type(ib) and isinstance(ib, MolObjective)
        assert ia.stats == ib.stats and "prior_launches" not in ib.stats
        for x, y in zip(ia[:6], ib[:6]):
            assert torch.equal(x, y)
        assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)


@pytest.mark.parametrize("objective,estimator", [("elbo", "reparam"), ("iwae", "reparam"), ("iwae", "dreg")])
@pytest.mark.parametrize("case,kind", TWO)
def test_the_standard_prior_is_the_call_without_a_prior(case, kind, objective, estimator):
    from ggpm_amd.prior import MixturePrior
    from ggpm_amd.property_vae import EstimatorObjective, MolObjective, PriorEstimatorObjective, PriorObjective
    c = _case(case, kind)
    g, model, batch, sch = c
    std = MixturePrior.standard(g.latent).to(DEV)
    kw = dict(n_samples=3, objective=objective, estimator=estimator, mol_weights=_weights(g, True),
              beta=0.3 if objective == "elbo" else 1.0)
    l0, i0, g0, _, _ = _step(model, None, case=c, **kw)
    l1, i1, g1, gp, _ = _step(model, std, case=c, **kw)
    assert type(i1) is (PriorEstimatorObjective if estimator == "dreg" else PriorObjective) and isinstance(i1, MolObjective)
    assert isinstance(i1, EstimatorObjective) == (estimator == "dreg") and len(i1) == 7
    assert rel_err(_np(l1), _np(l0)) <= 1e-6
    for what in ("kl", "elbo", "iwae"):
        assert rel_err(_np(getattr(i1, what)), _np(getattr(i0, what))) <= 1e-6, what
    assert torch.equal(i1.parts, i0.parts) and torch.equal(i1.z, i0.z) and torch.equal(i1.kl_standard, i0.kl)
    assert i1.log_prior_ratio.shape == (3, g.B) and float(i1.log_prior_ratio.abs().max()) <= 1e-9
    assert i1.stats == dict(i0.stats, prior_launches=3)                      # one forward, the row pass, the column pass
    assert set(g1) == set(g0)
    for k in g0:
        assert_close(_np(g1[k]), _np(g0[k]), "%s %s %s %s" % (case, objective, estimator, k), elem_tol=None)
    assert set(gp) == {"logits", "means", "log_vars"} and all(bool(torch.isfinite(v).all()) for v in gp.values())
    # log_likelihood under it
    a = model.log_likelihood(batch, n_samples=3, seed=SEED, schedule=sch)
    b = model.log_likelihood(batch, n_samples=3, seed=SEED, schedule=sch, prior=std)
    assert b.stats == dict(a.stats, prior_launches=1) and torch.equal(b.kl_standard, a.kl) and torch.equal(b.parts, a.parts)
    for what in ("kl", "elbo", "iwae"):
        assert rel_err(_np(getattr(b, what)), _np(getattr(a, what))) <= 1e-6, what
    # a frozen prior: no column pass
    for p in std.parameters():
        p.requires_grad_(False)
    _, i2, g2, gp2, _ = _step(model, std, case=c, **kw)
    assert i2.stats["prior_launches"] == 2 and not gp2 and all(torch.equal(g2[k], g1[k]) for k in g1)


# ---------------------------------------------------------------------------------------------- against the fp64 restatement
def _restated(c, prior, info, dz_dec, K, objective, estimator, w, beta):
    """-> (loss, {name: gradient}) of the latent chain in fp64 torch, the decoder entering through parts and J"""
    from ggpm_amd import functional as F_
    from ggpm_amd.latent_heads import _encode_heads
    from ggpm_amd.nnutils import make_cuda
    g, model, batch, sch = c
    B, L = g.B, g.latent
    with torch.no_grad():
        root, mean32, pv32 = _encode_heads(model, make_cuda(batch[2]))
    eps = F_.sample_latent_normal(K, B, L, SEED & 0xFFFFFFFF, SEED >> 32, device=DEV).double().cpu()
    f64 = lambda t: t.detach().double().cpu()
    mean, pv = f64(mean32).requires_grad_(), f64(pv32).requires_grad_()
    a, m, s = [f64(t).requires_grad_() for t in (prior.logits, prior.means, prior.log_vars)]
    wt = torch.ones(B, dtype=torch.float64) if w is None else torch.tensor(w, dtype=torch.float64)
    nll_run = f64(info.parts).sum(dim=2)                                     # [K, B]
    lv = -pv.abs()
    z = mean[None] + torch.exp(lv / 2)[None] * eps
    comp = torch.log_softmax(a, 0)[None, None] - 0.5 * (LOG_2PI + s[None, None] + (z[:, :, None] - m[None, None]) ** 2
                                                         * torch.exp(-s)[None, None]).sum(dim=3)
    ratio = torch.logsumexp(comp, dim=2) + 0.5 * (LOG_2PI + z * z).sum(dim=2)
    path = estimator != "reparam"
    mq, lq = (mean.detach(), lv.detach()) if path else (mean, lv)
    logpq = -0.5 * (z * z).sum(dim=2) + 0.5 * ((z - mq[None]) ** 2 * torch.exp(-lq)[None] + lq[None]).sum(dim=2) + ratio
    # the objective's coefficient of nll, in fp64, and with it J from what arrived at z_k
    with torch.no_grad():
        sw = torch.softmax(logpq - nll_run, dim=0)
        c_nll = wt[None] / (K * B) * torch.ones(K, 1, dtype=torch.float64) if objective == "elbo" else wt[None] * sw / B
        J = torch.stack([f64(d) for d in dz_dec]) / c_nll[:, :, None]
    nll = nll_run + (J * (z - z.detach())).sum(dim=2)
    if objective == "elbo":
        kl = -0.5 * (1 + lv - mean * mean - torch.exp(lv)).sum(dim=1)
        loss = (wt * (nll.mean(dim=0) + beta * (kl - ratio.mean(dim=0)))).sum() / B
    elif not path:
        loss = -(wt * (torch.logsumexp(logpq - nll, dim=0) - np.log(K))).sum() / B
    else:
        if estimator == "dreg":
            z.register_hook(lambda grad: grad * sw[:, :, None])
        loss = -(wt[None] * sw * (logpq - nll)).sum() / B
        value = -(wt * (torch.logsumexp((logpq - nll).detach(), dim=0) - np.log(K))).sum() / B
    loss.backward()
    H = model.R_mean.weight.shape[1]
    h = f64(root)[:, :H]
    grads = {"R_mean.weight": mean.grad.t() @ h, "R_mean.bias": mean.grad.sum(dim=0), "R_var.weight": pv.grad.t() @ h,
             "R_var.bias": pv.grad.sum(dim=0), "logits": a.grad, "means": m.grad, "log_vars": s.grad}
    return (value if path else loss.detach()), {k: v.numpy() for k, v in grads.items()}, _np(ratio)


CHAIN = [("elbo", "reparam", 1), ("elbo", "reparam", 3), ("iwae", "reparam", 3), ("iwae", "stl", 3), ("iwae", "dreg", 3)]


@pytest.mark.parametrize("objective,estimator,K", CHAIN)
@pytest.mark.parametrize("case,kind", TWO)
def test_a_three_component_prior_against_the_fp64_restatement(case, kind, objective, estimator, K):
    c = _case(case, kind)
    g, model, batch, sch = c
    prior = _prior(g)
    w, beta = _weights(g, True), 0.3 if objective == "elbo" else 1.0
    loss, info, gm, gp, dz_dec = _step(model, prior, case=c, n_samples=K, objective=objective, estimator=estimator, mol_weights=w,
                                      beta=beta)
    assert len(dz_dec) == K and info.stats["prior_launches"] == 3 and info.stats["decoder_passes"] == K
    want_loss, want, ratio = _restated(c, prior, info, dz_dec, K, objective, estimator, w, beta)
    e = rel_err(_np(loss), _np(want_loss))
    print("%s %s %s K %d: loss %.3e" % (case, objective, estimator, K, e))
    assert e < PARITY
    assert rel_err(_np(info.log_prior_ratio), ratio) < PARITY and float(np.abs(ratio).max()) > 0.1
    assert rel_err(_np(info.kl), _np(info.kl_standard) - ratio.mean(axis=0)) < PARITY
    for k, wv in want.items():
        got = _np(gp[k]) if k in gp else _np(gm[k])
        assert np.isfinite(got).all() and np.abs(wv).max() > 0
        e = rel_err(got, wv)
        print("%s %s %s K %d: %s %.3e" % (case, objective, estimator, K, k, e))
        assert e < PARITY, (k, e)
    # log_likelihood under the same prior, the same draws: bound_loss's fields
    ll = model.log_likelihood(batch, n_samples=K, seed=SEED, schedule=sch, prior=prior)
    for what in ("kl", "elbo", "iwae", "log_prior_ratio", "kl_standard"):
        assert rel_err(_np(getattr(ll, what)), _np(getattr(info, what))) <= 1e-6, what


def test_what_a_prior_excludes_raises_and_a_second_backward_does():
    from ggpm_amd.prior import MixturePrior
    c = _case(*TWO[0])
    g, model, batch, sch = c
    prior = _prior(g)
    model.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match="standard normal"):
        model.bound_loss(batch, free_bits=0.1, prior=prior, schedule=sch)
    with pytest.raises(ValueError, match="standard normal"):
        model.bound_loss(batch, objective="tcvae", dataset_size=1000, prior=prior, schedule=sch)
    with pytest.raises(ValueError, match="latent columns"):
        model.bound_loss(batch, prior=MixturePrior(2, g.latent + 1).to(DEV), schedule=sch)
    with pytest.raises(ValueError, match="the prior is on"):
        model.bound_loss(batch, prior=MixturePrior(2, g.latent), schedule=sch)
    with pytest.raises(ValueError, match="MixturePrior"):
        model.log_likelihood(batch, prior="mixture", schedule=sch)
    with pytest.raises(ValueError, match="latent columns"):
        model.sample(2, seed=1, prior=MixturePrior(2, g.latent + 1).to(DEV))
    z = torch.randn(4, g.latent, device=DEV, requires_grad=True)
    out = prior.log_prob(z).sum()
    out.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a retained graph is not supported"):
        out.backward()
    assert z.grad.shape == z.shape and prior.responsibilities(z).shape == (4, 3) and not prior.responsibilities(z).requires_grad
    assert float((prior.responsibilities(z).sum(dim=1) - 1).abs().max()) <= 1e-6
    assert prior.log_ratio(z.detach().reshape(2, 2, g.latent)).shape == (2, 2)


# ---------------------------------------------------------------------------------------------- sample
@pytest.mark.parametrize("kind", ["motif", "hier"])
def test_sample_with_a_prior_decodes_its_draws(kind):
    import sampled_decode_fixtures as SF
    from decode_fixtures import norm
    from test_sampled_decode_gpu import _hier, _motif
    from ggpm_amd.prior import MixturePrior
    m = _motif("prop_lstm_s61") if kind == "motif" else _hier("prop", "vae_gru_s42")
    gb, seed, steps = SF.graph_batch(kind), 0xABCDEF0123456789, 12
    torch.manual_seed(11)
    p = MixturePrior(3, m.decoder.latent_size, init_std=1.5).to(DEV)
    z, comp = p.sample(4, seed=seed, return_components=True)
    assert z.shape == (4, m.decoder.latent_size) and comp.dtype == torch.int32 and torch.equal(p.sample(4, seed=seed), z)
    want = m.decoder.decode(None, (z, z, z), max_decode_step=steps, graph_batch_factory=gb)
    assert norm(m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb, prior=p)) == norm(want)
    a = m.sample(4, greedy=False, seed=seed, max_decode_step=steps, graph_batch_factory=gb, prior=p)
    assert norm(a) == norm(m.decoder.decode_sampled(None, (z, z, z), seed=seed, max_decode_step=steps, graph_batch_factory=gb))
    # prior=None: the standard-normal draws, as without the argument
    base = m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb)
    assert norm(m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb, prior=None)) == norm(base)
    std = MixturePrior.standard(m.decoder.latent_size).to(DEV)
    assert norm(m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb, prior=std)) == norm(base)


# ---------------------------------------------------------------------------------------------- a post-hoc fit
def _oracle_fit(z, a, m, s, steps, lr):
    """torch Adam's update restated in numpy fp64 on the oracle's loss -mean logp and its gradients -> the losses"""
    p = [np.array(x, np.float64) for x in (a, m, s)]
    mo, ve, losses = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p], []
    g = np.full(len(z), -1.0 / len(z))
    for t in range(1, steps + 1):
        losses.append(float(-O.forward(z, *p)["logp"].mean()))
        _, dm, ds, da = O.backward(z, p[0], p[1], p[2], g, True)
        for i, gr in enumerate((da, dm, ds)):
            mo[i] = 0.9 * mo[i] + 0.1 * gr
            ve[i] = 0.999 * ve[i] + 0.001 * gr * gr
            p[i] = p[i] - lr * (mo[i] / (1 - 0.9 ** t)) / (np.sqrt(ve[i] / (1 - 0.999 ** t)) + 1e-8)
    losses.append(float(-O.forward(z, *p)["logp"].mean()))
    return losses


def test_twenty_adam_steps_on_fixed_latents_lower_the_loss_as_the_oracle_does():
    """A smoke check of the training direction, not a tolerance: z is drawn by the oracle from a known two-component mixture"""
    from ggpm_amd.prior import MixturePrior
    L, N, lr = 6, 256, 0.05
    ta, tm, ts = np.zeros(2), np.stack([np.full(L, -2.0), np.full(L, 2.0)]), np.full((2, L), -1.0)
    z64, _ = O.sample(77, np.arange(N), ta, tm, ts)
    z32 = z64.astype(np.float32)
    torch.manual_seed(1)
    prior = MixturePrior(2, L, init_std=0.5)
    start = [t.detach().numpy().copy() for t in (prior.logits, prior.means, prior.log_vars)]
    want = _oracle_fit(z32.astype(np.float64), *start, steps=20, lr=lr)
    prior = prior.to(DEV)
    z = torch.from_numpy(z32).to(DEV)
    opt = torch.optim.Adam(prior.parameters(), lr=lr)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = -prior.log_prob(z).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(-prior.log_prob(z).mean()))
    print("fit: %.4f -> %.4f (oracle %.4f -> %.4f)" % (losses[0], losses[-1], want[0], want[-1]))
    assert all(losses[i + 1] < losses[i] for i in range(5))
    assert want[0] - want[-1] > 0
    assert losses[0] - losses[-1] >= (want[0] - want[-1]) * 0.99
