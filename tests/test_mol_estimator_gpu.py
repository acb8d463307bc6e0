"""GPU: ``bound_loss(objective="iwae", estimator="stl" | "dreg")`` of the four VAEs end to end, on the fixtures of
tests/mol_likelihood_fixtures.py with K = 3 draws of a fixed seed, unweighted and weighted.  The reference has no such
estimator.  What does not depend on the estimator -- the loss, ``info``'s seven fields, the gradient of every parameter only the
decoder uses -- is compared bit for bit with ``estimator="reparam"``; every gradient is compared, under the project's 1e-4
norm-wise, with a composite of existing pieces: the posterior and z_k in torch ops under autograd, the decoder's
``molecule_losses`` per draw over one recorded atom level, and the surrogate loss of tests/test_mol_estimator_cpu.py (the
normalised weights held constant, log q's parameters detached, for DReG a hook that weighs what arrives at z_k by s_k)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import mol_estimator_oracle as E
import mol_likelihood_fixtures as LF
from golden_utils import rel_err
from test_latent_dims_gpu import FOUR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4           # the project's relative parity figure (BASELINE.json)
SEED = 0x1234ABCD5678EF01
K = 3
SEVEN = ("parts", "kl", "elbo", "iwae", "z", "weights")


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    g = LF.LLGolden(case)
    batch, sch = g.batch()
    return g, g.model(kind).to(DEV), batch, sch


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _weights(g, weighted):
    return [float(v) for v in np.linspace(0.5, 2.0, g.B)] if weighted else None


def _grads(model):
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _step(model, fn):
    """zero_grad, ``fn() -> (loss, info)``, backward -> (loss, info, {first name: gradient})"""
    model.zero_grad(set_to_none=True)
    loss, info = fn()
    loss.backward()
    return loss.detach().clone(), info, _grads(model)


@functools.lru_cache(maxsize=None)
def _bound(case, kind, weighted, estimator, n_samples=K):
    """One ``bound_loss`` + backward of the case, computed once and shared (nothing changes it)"""
    g, model, batch, sch = _case(case, kind)
    out = _step(model, lambda: model.bound_loss(batch, n_samples=n_samples, objective="iwae", mol_weights=_weights(g, weighted),
                                                seed=SEED, schedule=sch, estimator=estimator))
    model.zero_grad(set_to_none=True)
    return out


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
    return worst


def _eps(g):
    from ggpm_amd import functional as F_
    return F_.sample_latent_normal(K, g.B, g.latent, SEED & 0xFFFFFFFF, SEED >> 32, device=DEV)


def _posterior(model, tensors):
    """(mean, pre_var) [B, L] with gradients: the encoder's own launches, the two heads in torch ops"""
    root = model._encode(tensors)
    H = model.R_mean.weight.shape[1]
    return (TF.linear(root[:, :H], model.R_mean.weight, model.R_mean.bias),
            TF.linear(root[:, :H], model.R_var.weight, model.R_var.bias))


def _composite(case, kind, weighted, estimator):
    """The surrogate loss over existing pieces + backward -> {first name: gradient}"""
    from ggpm_amd.decoder import _pinned_cls_size
    from ggpm_amd.nnutils import make_cuda
    g, model, batch, sch = _case(case, kind)
    mols, graphs, tensors, orders = batch[0], batch[1], make_cuda(batch[2]), batch[3]
    w = _weights(g, weighted)
    wt = torch.ones(g.B, device=DEV) if w is None else torch.tensor(w, dtype=torch.float32, device=DEV)
    eps = _eps(g)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        atom = model.decoder.atom_level(sch, tensors, record_grad=True) if model.HIER else None
        mean, pv = _posterior(model, tensors)
        lv = -pv.abs()
        zs, lws = [], []
        for k in range(K):
            zk = mean + torch.exp(lv / 2) * eps[k]
            zs.append(zk)
            parts = model.decoder.molecule_losses(mols, (zk, zk, zk), graphs, tensors, orders, schedule=sch,
                                                  max_cls_size=_pinned_cls_size(sch, None), atom=atom)
            nll = (parts[:, 0] + parts[:, 1]) + (parts[:, 2] + parts[:, 3])
            lws.append(-0.5 * (zk * zk).sum(dim=1)
                       + 0.5 * ((zk - mean.detach()) ** 2 * torch.exp(-lv.detach()) + lv.detach()).sum(dim=1) - nll)
        lw = torch.stack(lws)
        s = torch.softmax(lw.detach().double(), dim=0).float()
        if estimator == "dreg":
            for k in range(K):
                zs[k].register_hook(lambda grad, k=k: grad * s[k][:, None])
        loss = -(wt[None] * s * lw).sum() / g.B
    loss.backward()
    grads = _grads(model)
    model.zero_grad(set_to_none=True)
    return grads


# ---------------------------------------------------------------------------------------------- against "reparam"
@pytest.mark.parametrize("estimator", ["stl", "dreg"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case,kind", FOUR)
def test_what_the_estimator_does_not_touch_is_bit_equal_to_reparam(case, kind, weighted, estimator):
    from ggpm_amd.property_vae import EstimatorObjective, MolObjective
    g, model, batch, sch = _case(case, kind)
    want_loss, plain, want = _bound(case, kind, weighted, "reparam")
    got_loss, info, got = _bound(case, kind, weighted, estimator)
    assert torch.equal(got_loss, want_loss)
    assert type(plain) is MolObjective and type(info) is EstimatorObjective and isinstance(info, MolObjective) and len(info) == 7
    for what in SEVEN:
        a = getattr(info, what)
        assert torch.equal(a, getattr(plain, what)), what
        assert not a.requires_grad and a.dtype == torch.float32
    assert info.stats == plain.stats == dict(encoder_calls=1, atom_level_calls=1 if g.decoder == "hier" else 0, decoder_passes=K)
    assert info.estimator == estimator
    for a, shape in ((info.sample_weights, (K, g.B)), (info.ess, (g.B,))):
        assert tuple(a.shape) == shape and a.dtype == torch.float32 and a.is_cuda and not a.requires_grad
    # the parameters neither the encoder nor the latent heads use: their gradient is the decoder's, with the coefficient c
    upstream = {id(p) for m in (model.encoder, model.R_mean, model.R_var) for p in m.parameters()}
    untouched = [k for k, p in model.named_parameters() if id(p) not in upstream and k in want]
    assert len(untouched) >= 10 and set(got) == set(want)
    for k in untouched:
        assert torch.equal(got[k], want[k]), k
    moved = [k for k in want if k not in untouched and not torch.equal(got[k], want[k])]
    assert any(k.startswith("R_mean.") for k in moved) and any(k.startswith("R_var.") for k in moved)
    print("%s %s w %d %s: %d gradients bit-equal to reparam's, %d differ" % (case, kind, weighted, estimator, len(untouched), len(moved)))


# ---------------------------------------------------------------------------------------------- against the composite
@pytest.mark.parametrize("estimator", ["stl", "dreg"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case,kind", FOUR)
def test_gradients_against_the_composite_of_existing_pieces(case, kind, weighted, estimator):
    _, _, got = _bound(case, kind, weighted, estimator)
    want = _composite(case, kind, weighted, estimator)
    _check_grads(got, want, "%s %s w %d %s against the composite" % (case, kind, weighted, estimator))


# ---------------------------------------------------------------------------------------------- further checks
@pytest.mark.parametrize("case,kind", FOUR)
def test_one_sample_makes_dreg_and_stl_the_same(case, kind):
    _, a_info, a = _bound(case, kind, True, "stl", 1)
    _, b_info, b = _bound(case, kind, True, "dreg", 1)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert bool((b_info.sample_weights == 1.0).all()) and bool((b_info.ess == 1.0).all())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case,kind", FOUR)
def test_sample_weights_and_ess_are_the_oracles(case, kind, weighted):
    """logpq re-formed in fp64 from ``info.z``, the draws and the posterior's lv.  The kernel reads the fp32 logpq and parts:
    a log-weight of size |lw| carries up to a few fp32 roundings, so a weight is off by about 1e-6 |lw| relative -- far inside
    the project's 1e-4, which is asserted."""
    from ggpm_amd.nnutils import make_cuda
    g, model, batch, sch = _case(case, kind)
    _, info, _ = _bound(case, kind, weighted, "dreg")
    with torch.no_grad():
        mean, pv = _posterior(model, make_cuda(batch[2]))
    z, eps, lv = _np(info.z), _np(_eps(g)), -np.abs(_np(pv))
    logpq = -0.5 * (z * z).sum(axis=2) + 0.5 * (eps * eps + lv[None]).sum(axis=2)
    s64, ess64 = E.iwae_weights(_np(info.parts), logpq)
    s, ess = _np(info.sample_weights), _np(info.ess)
    es, ee = rel_err(s, s64), rel_err(ess, ess64)
    print("%s %s w %d: sample_weights %.3e, ess %.3e (ess %s)" % (case, kind, weighted, es, ee, np.round(ess, 3)))
    assert es < PARITY and ee < PARITY
    assert (ess >= 1.0).all() and (ess <= K).all()
    assert np.abs(s.sum(axis=0) - 1.0).max() <= K * 2.0 ** -23


@pytest.mark.parametrize("estimator", ["stl", "dreg"])
@pytest.mark.parametrize("side", ["0", "1"])
@pytest.mark.parametrize("case,kind", [("ll_hier_lstm_s41", "hier-prop-opt"), ("ll_motif_lstm_s61", "prop-opt")])
def test_a_second_step_adds_into_grad(case, kind, side, estimator, monkeypatch):
    """no zero_grad between two bound_loss(estimator=) + backward: every .grad is twice the single-pass gradient within 1e-6
    relative (tied embedding tables included), and stays the tensor it was"""
    monkeypatch.setenv("GGPM_SIDE_STREAM", side)
    g, model, batch, sch = _case(case, kind)
    fn = lambda: model.bound_loss(batch, n_samples=2, objective="iwae", mol_weights=_weights(g, True), seed=SEED, schedule=sch,
                                  estimator=estimator)
    _, _, once = _step(model, fn)
    held = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    fn()[0].backward()
    torch.cuda.synchronize()
    worst = 0.0
    for k, p in model.named_parameters():
        if k in once:
            assert p.grad is held[k], k
            e = rel_err(_np(p.grad), 2 * _np(once[k]))
            worst = max(worst, e)
            assert e <= 1e-6, (k, e)
    print("%s %s side %s %s: two passes against twice one, largest distance %.3e" % (case, kind, side, estimator, worst))
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("estimator", ["stl", "dreg"])
@pytest.mark.parametrize("case,kind", [("ll_hier_gru_s40", "hier-prop"), ("ll_motif_lstm_s61", "prop-opt")])
def test_second_backward_raises(case, kind, estimator):
    g, model, batch, sch = _case(case, kind)
    model.zero_grad(set_to_none=True)
    loss, _ = model.bound_loss(batch, n_samples=2, objective="iwae", seed=SEED, schedule=sch, estimator=estimator)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a retained graph is not supported"):
        loss.backward()
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)


def test_argument_errors():
    g, model, batch, sch = _case("ll_hier_gru_s40", "hier-prop")
    model.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match="estimator"):
        model.bound_loss(batch, objective="elbo", estimator="dreg", schedule=sch)
    with pytest.raises(ValueError, match="estimator"):
        model.bound_loss(batch, estimator="stl", schedule=sch)                       # the default objective is the ELBO
    with pytest.raises(ValueError, match=r"reparam, stl, dreg"):
        model.bound_loss(batch, objective="iwae", estimator="score", schedule=sch)
    for objective in ("elbo", "iwae"):
        with pytest.raises(ValueError):
            model.bound_loss(batch, objective=objective, estimator="dreg", free_bits=0.1, schedule=sch)
    with pytest.raises(ValueError, match="beta"):                                    # what was refused before still is
        model.bound_loss(batch, objective="iwae", beta=0.5, estimator="dreg", schedule=sch)
    m2 = g.model("hier-prop", dropout=0.1).to(DEV)
    m2.train()
    with pytest.raises(NotImplementedError, match=r"bound_loss runs without dropout: call model\.eval\(\) first"):
        m2.bound_loss(batch, objective="iwae", estimator="dreg", schedule=sch)
    assert all(p.grad is None for p in model.parameters())
