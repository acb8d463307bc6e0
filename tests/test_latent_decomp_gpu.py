"""GPU: ``bound_loss(objective="tcvae")``, ``latent_decomposition`` and ``latent_decomposition_accumulator`` of the VAEs end
to end, on the fixtures of tests/mol_likelihood_fixtures.py (one hierarchical GRU, one hierarchical LSTM, one tree-only model).
The reference has no split of the KL.  With alpha = beta = gamma = 1 the loss is the single-sample estimate of the ELBO and is
compared with a composite of existing pieces, ``bound_loss("elbo", beta=0)`` plus the weighted mean of -logpq of the existing
latent terms; with unequal weights the latent part is compared with tests/latent_decomp_oracle.py (fp64, its backward chained
through the fp64 rsample) on the model's own posterior parameters and draws.  PARITY = 1e-4, norm-wise, as in
tests/test_latent_dims_gpu.py.

The bound of ``mi + tc + dwkl = -logpq``: the three components are fp64 sums rounded once each, u (|mi| + |tc| + |dwkl|); logpq
is a fp64 sum rounded once, u |logpq|, but it takes (z - mean)^2 exp(-lv) to be eps^2, while the split reads the STORED fp32
z = fl(mean + fl(exp(lv / 2)) eps): z is off by u |z| for its rounding and 3 u |d| for the product and expf, d = z - mean, so
d^2 exp(-lv) / 2 is off by exp(-lv) |d| u (|z| + 3 |d|) per column."""
import functools

import numpy as np
import pytest
import torch

import latent_decomp_oracle as O
import mol_likelihood_fixtures as LF
from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4
U = 2.0 ** -24
SEED = 0x1234ABCD5678EF01
THREE = [("ll_hier_gru_s40", "hier-prop"), ("ll_hier_lstm_s41", "hier-prop"), ("ll_motif_gru_s60", "prop")]
HEADS = ("R_mean.weight", "R_mean.bias", "R_var.weight", "R_var.bias")
WEIGHTS = dict(alpha=0.7, beta=4.0, gamma=1.3)
R_MEAN_SCALE = 0.1          # applied to R_mean where a fixture's own posteriors do not overlap (see _case)
N_DATA = 250000


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _posterior(model, batch):
    from ggpm_amd.nnutils import make_cuda
    from ggpm_amd.latent_heads import _latent_heads
    with torch.no_grad():
        root = model._encode(make_cuda(batch[2]))
        mean, pv = _latent_heads(root, model.R_mean.weight, model.R_mean.bias, model.R_var.weight, model.R_var.bias)
    return root, mean, pv


def _eps(K, B, L, first_id=0):
    from ggpm_amd import functional as F_
    from ggpm_amd.greedy_decode import split_seed
    lo, hi = split_seed(SEED)
    ids = torch.arange(first_id, first_id + B, dtype=torch.int64)
    return F_.sample_latent_normal(K, B, L, lo, hi, ids=ids, device=DEV)


def _off_diagonal_mass(model, batch, K=3):
    _, mean, pv = _posterior(model, batch)
    eps = _eps(K, mean.shape[0], mean.shape[1])
    f = O.forward(O.rsample(_np(mean), _np(pv), _np(eps)), _np(mean), _np(pv), 0.0)
    B = mean.shape[0]
    return float((1.0 - f["p"][:, np.arange(B), np.arange(B)]).max())


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """the fixture's model, with R_mean scaled by R_MEAN_SCALE if its posteriors do not overlap: the tests below must see the
    cross terms, so some draw must give another molecule's posterior more than 1e-3 of the softmax mass"""
    g = LF.LLGolden(case)
    batch, sch = g.batch()
    model = g.model(kind).to(DEV)
    mass = _off_diagonal_mass(model, batch)
    if mass <= 1e-3:
        with torch.no_grad():
            model.R_mean.weight.mul_(R_MEAN_SCALE)
            model.R_mean.bias.mul_(R_MEAN_SCALE)
        mass = _off_diagonal_mass(model, batch)
    print("%s %s: largest off-diagonal mass 1 - p_ii %.3e" % (case, kind, mass))
    assert mass > 1e-3
    return g, model, batch, sch


def _step(model, fn):
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _check_grads(got, want, what):
    """Every tensor within PARITY norm-wise of ``want``'s; a tensor whose wanted gradient is below 1e-6 of the largest:
    max|got| <= PARITY gmax.  The two sets of parameters must be the same."""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    got, want = {k: _np(v) for k, v in got.items()}, {k: _np(v) for k, v in want.items()}
    gmax = max(np.abs(v).max() for v in want.values())
    worst = 0.0
    for k, w in want.items():
        a = got[k]
        if np.abs(w).max() < 1e-6 * gmax:
            assert np.abs(a).max() <= PARITY * gmax, (what, k, np.abs(a).max(), gmax)
            continue
        e = rel_err(a, w)
        worst = max(worst, e)
        assert e < PARITY, (what, k, e)
    print("%s: %d gradients, largest distance %.3e" % (what, len(want), worst))


def _weights(g, weighted):
    return [float(v) for v in np.linspace(0.5, 2.0, g.B)] if weighted else None


# ---------------------------------------------------------------------------------------------- alpha = beta = gamma = 1
@pytest.mark.parametrize("case,kind", THREE)
def test_equal_weights_against_the_composite_of_existing_pieces(case, kind):
    from ggpm_amd.nnutils import make_cuda
    from ggpm_amd.latent_heads import _LatentTerms
    g, model, batch, sch = _case(case, kind)
    K = 2
    w = _weights(g, True)
    wt = torch.tensor(w, dtype=torch.float32, device=DEV)
    kw = dict(n_samples=K, mol_weights=w, seed=SEED, schedule=sch)
    # the composite: bound_loss(beta=0) and the weighted mean of -logpq of the existing latent terms, two passes into .grad
    model.zero_grad(set_to_none=True)
    l0 = model.bound_loss(batch, objective="elbo", beta=0.0, **kw)[0]
    l0.backward()
    torch.cuda.synchronize()
    Rm, Rv = model.R_mean, model.R_var
    with torch.enable_grad():
        root = model._encode(make_cuda(batch[2]))
        _, _, logpq = _LatentTerms.apply(root, Rm.weight, Rm.bias, Rv.weight, Rv.bias, _eps(K, g.B, g.latent))
        term = -(logpq.mean(dim=0) * wt).sum() / g.B
    term.backward()
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    want_loss = float(l0.detach()) + float(term.detach())
    for N in (g.B, N_DATA):
        got_loss, got = _step(model, lambda: model.bound_loss(batch, objective="tcvae", beta=1.0, dataset_size=N, **kw)[0])
        print("%s %s N %d: loss %.9g, composite %.9g" % (case, kind, N, float(got_loss), want_loss))
        assert abs(float(got_loss) - want_loss) <= PARITY * abs(want_loss)
        _check_grads(got, want, "%s %s N %d equal weights against the composite" % (case, kind, N))
    model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------- unequal weights
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case,kind", THREE)
def test_unequal_weights_against_the_oracle_chained_through_the_rsample(case, kind, weighted, K):
    from ggpm_amd import functional as F_
    from ggpm_amd.nnutils import make_cuda
    g, model, batch, sch = _case(case, kind)
    w = _weights(g, weighted)
    kw = dict(n_samples=K, mol_weights=w, seed=SEED, schedule=sch)
    base_loss, base = _step(model, lambda: model.bound_loss(batch, objective="elbo", beta=0.0, **kw)[0])
    _, plain = model.bound_loss(batch, objective="elbo", beta=1.0, **kw)
    model.zero_grad(set_to_none=True)
    loss, info = model.bound_loss(batch, objective="tcvae", dataset_size=N_DATA, **WEIGHTS, **kw)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    # the oracle on the model's own posterior parameters and draws
    root, mean, pv = _posterior(model, batch)
    eps = _eps(K, g.B, g.latent)
    c = O.log_nb(N_DATA, g.B)
    term, dm, dp, f = O.tcvae_term(_np(mean), _np(pv), _np(eps), w, WEIGHTS["alpha"], WEIGHTS["beta"], WEIGHTS["gamma"], c)
    mass = float((1.0 - f["p"][:, np.arange(g.B), np.arange(g.B)]).max())
    print("%s %s K %d w %d: off-diagonal mass %.3e; loss %.9g, beta=0 loss + oracle term %.9g"
          % (case, kind, K, weighted, mass, float(loss.detach()), float(base_loss) + term))
    assert mass > 1e-3                                               # the cross terms are there to be seen
    assert abs(float(loss.detach()) - (float(base_loss) + term)) <= PARITY * abs(float(base_loss) + term)
    for what in ("mi", "tc", "dwkl"):
        a = getattr(info, what)
        assert a.shape == (K, g.B) and a.dtype == torch.float32 and not a.requires_grad
        e = rel_err(_np(a), f[what])
        print("    %s: %.3e" % (what, e))
        assert e < PARITY, (what, e)

    # info: the seven fields of the "elbo" call, bit for bit
    assert len(info) == 7
    for what in ("parts", "kl", "elbo", "iwae", "z", "weights"):
        assert torch.equal(getattr(info, what), getattr(plain, what)), what
    assert info.stats == plain.stats
    assert (info.alpha, info.beta, info.gamma, info.dataset_size) == (0.7, 4.0, 1.3, N_DATA)

    # mi + tc + dwkl = -logpq of the existing latent terms, within the bound of the docstring
    z32, _, logpq = F_.latent_terms(mean, pv, eps)
    assert torch.equal(z32, info.z)
    zz, mm, iv = _np(z32), _np(mean), np.exp(np.abs(_np(pv)))
    d = np.abs(zz - mm[None])
    bound = U * (np.abs(_np(info.mi)) + np.abs(_np(info.tc)) + np.abs(_np(info.dwkl)) + np.abs(_np(logpq))) \
        + (iv[None] * d * U * (np.abs(zz) + 3 * d)).sum(axis=2)
    s = _np(info.mi) + _np(info.tc) + _np(info.dwkl)
    err = np.abs(s + _np(logpq))
    print("    mi + tc + dwkl + logpq: %.3e (bound %.3e)" % (err.max(), bound.max()))
    assert (err <= bound * (1 + 2.0 ** -10)).all()

    # the latent heads' share by itself, and every gradient as the beta = 0 pass plus the oracle's share
    H = model.R_mean.weight.shape[1]
    h = _np(root[:, :H])
    share = {"R_mean.weight": dm.T @ h, "R_mean.bias": dm.sum(axis=0), "R_var.weight": dp.T @ h, "R_var.bias": dp.sum(axis=0)}
    for k in HEADS:
        e = rel_err(_np(got[k]) - _np(base[k]), share[k])
        print("    d%s, the split KL's share: %.3e" % (k, e))
        assert e < PARITY, (k, e)
    d_root = torch.zeros_like(root)
    d_root[:, :H] = torch.from_numpy(dm @ _np(model.R_mean.weight) + dp @ _np(model.R_var.weight)).to(DEV, torch.float32)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        model._encode(make_cuda(batch[2])).backward(d_root)
    torch.cuda.synchronize()
    enc = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert enc and not set(enc) & set(HEADS)
    want = {}
    for k, v in base.items():
        want[k] = v.double()
        if k in enc:
            want[k] = want[k] + enc[k].double()
        if k in share:
            want[k] = want[k] + torch.from_numpy(share[k]).to(DEV)
    _check_grads(got, want, "%s %s K %d w %d unequal weights" % (case, kind, K, weighted))
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("case,kind", [("ll_hier_lstm_s41", "hier-prop"), ("ll_motif_gru_s60", "prop")])
def test_a_second_step_adds_into_grad_and_a_second_backward_raises(case, kind):
    g, model, batch, sch = _case(case, kind)
    kw = dict(n_samples=2, objective="tcvae", dataset_size=N_DATA, mol_weights=_weights(g, True), seed=SEED, schedule=sch, **WEIGHTS)
    fn = lambda: model.bound_loss(batch, **kw)[0]
    _, once = _step(model, fn)
    held = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    fn().backward()
    torch.cuda.synchronize()
    twice = {}
    for k, p in model.named_parameters():
        if k in once:
            assert p.grad is held[k], k
            twice[k] = p.grad.clone()
    _check_grads(twice, {k: 2 * v for k, v in once.items()}, "%s %s two passes against twice one" % (case, kind))
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a retained graph is not supported"):
        loss.backward()
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------- the diagnostic
@pytest.mark.parametrize("case,kind", THREE)
def test_latent_decomposition_over_two_batches_is_the_oracle_on_both(case, kind):
    from ggpm_amd import functional as F_
    from ggpm_amd.property_vae import LatentDecomposition
    g, model, batch, sch = _case(case, kind)
    K, B, L = 3, g.B, g.latent
    res = model.latent_decomposition([batch, batch], N_DATA, n_samples=K, seed=SEED)
    assert type(res) is LatentDecomposition and res.n_molecules == 2 * B and type(res.n_molecules) is int
    _, mean, pv = _posterior(model, batch)
    c = O.log_nb(N_DATA, B)
    fs = []
    for first in (0, B):                                             # molecule n of the pass has sample id n
        z, _, _ = F_.latent_terms(mean, pv, _eps(K, B, L, first))
        fs.append(O.forward(_np(z), _np(mean), _np(pv), c))
    assert not np.array_equal(fs[0]["mi"], fs[1]["mi"])
    want = {k: np.concatenate([f[k].reshape(K * B, -1) for f in fs]).mean(axis=0) for k in ("mi", "tc", "dwkl", "dwkl_dim")}
    for what, key in (("mi", "mi"), ("tc", "tc"), ("dwkl", "dwkl"), ("dwkl_dims", "dwkl_dim")):
        a = getattr(res, what)
        assert a.dtype == torch.float32 and a.is_cuda and not a.requires_grad and a.shape == (() if what != "dwkl_dims" else (L,))
        e = rel_err(_np(a).reshape(-1), want[key])
        print("%s %s %s: %.9g, oracle %.9g, distance %.3e" % (case, kind, what, float(_np(a).sum()), float(want[key].sum()), e))
        assert e < PARITY, (what, e)
    one = model.latent_decomposition([batch], N_DATA, n_samples=K, seed=SEED)
    assert rel_err(np.array([float(one.mi)]), np.array([fs[0]["mi"].mean()])) < PARITY
    assert not torch.equal(one.mi, res.mi)                           # the second batch did not reuse the first one's draws
    kl = float(_np(model.log_likelihood(batch, n_samples=1, seed=SEED, schedule=sch).kl).mean())
    assert abs(float(res.kl) - kl) <= PARITY * abs(kl) and res.kl.dim() == 0
    # update, read, update, read: the accumulator gives the same bits as the two calls above
    acc = model.latent_decomposition_accumulator(N_DATA, n_samples=K, seed=SEED)
    assert acc.result().n_molecules == 0 and float(acc.result().mi) == 0.0
    first = acc.update(batch).result()
    second = acc.update(batch).result()
    for what in ("mi", "tc", "dwkl", "dwkl_dims", "kl"):
        assert torch.equal(getattr(first, what), getattr(one, what)), what
        assert torch.equal(getattr(second, what), getattr(res, what)), what


def test_a_model_with_active_dropout_is_refused():
    g, model, batch, sch = _case("ll_hier_gru_s40", "hier-prop")
    m2 = g.model("hier-prop", dropout=0.1).to(DEV)
    m2.train()
    with pytest.raises(NotImplementedError, match=r"latent_decomposition runs without dropout: call model\.eval\(\) first"):
        m2.latent_decomposition([batch], N_DATA)
    with pytest.raises(NotImplementedError, match=r"runs without dropout"):
        m2.latent_decomposition_accumulator(N_DATA)
    acc = m2.eval().latent_decomposition_accumulator(N_DATA)
    m2.train()
    with pytest.raises(NotImplementedError, match=r"runs without dropout"):
        acc.update(batch)
    assert acc.n_molecules == 0 and not bool(acc.acc.ne(0).any())
    with pytest.raises(NotImplementedError, match=r"runs without dropout"):
        m2.bound_loss(batch, objective="tcvae", dataset_size=N_DATA, schedule=sch)


def test_argument_errors():
    g, model, batch, sch = _case("ll_hier_gru_s40", "hier-prop")
    tc = dict(objective="tcvae", schedule=sch)
    with pytest.raises(ValueError, match="dataset_size"):
        model.bound_loss(batch, **tc)
    with pytest.raises(ValueError, match="dataset_size"):
        model.bound_loss(batch, dataset_size=g.B - 1, **tc)
    with pytest.raises(ValueError, match="dataset_size"):
        model.bound_loss(batch, dataset_size=float(N_DATA), **tc)
    for est in ("stl", "dreg"):
        with pytest.raises(ValueError, match="estimator"):
            model.bound_loss(batch, dataset_size=N_DATA, estimator=est, **tc)
    with pytest.raises(ValueError, match="free_bits"):
        model.bound_loss(batch, dataset_size=N_DATA, free_bits=0.1, **tc)
    for name in ("alpha", "beta", "gamma"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=name):
                model.bound_loss(batch, dataset_size=N_DATA, **{name: bad}, **tc)
    for objective in ("elbo", "iwae"):
        for extra in (dict(alpha=1.0), dict(gamma=2.0), dict(dataset_size=N_DATA)):
            with pytest.raises(ValueError, match="tcvae"):
                model.bound_loss(batch, objective=objective, schedule=sch, **extra)
    for objective in ("vae", "free_bits"):                                    # what was refused before still is
        with pytest.raises(ValueError, match="objective"):
            model.bound_loss(batch, objective=objective, schedule=sch)
    with pytest.raises(ValueError, match="dataset_size"):
        model.latent_decomposition([batch], g.B - 1)
    with pytest.raises(ValueError, match="dataset_size"):
        model.latent_decomposition_accumulator(0)
    with pytest.raises(ValueError, match="n_samples"):
        model.latent_decomposition_accumulator(N_DATA, n_samples=0)
    assert all(p.grad is None for p in model.parameters())
