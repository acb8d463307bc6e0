"""GPU: ``bound_loss`` of the four VAEs end to end -- loss and every parameter gradient against the reference's (the fixtures
of tests/golden/make_golden_mol_objective.py), against the training step of the same model, against ``log_likelihood`` for
what ``info`` reports, and for determinism, accumulation into ``.grad``, the second backward and the argument errors."""
import functools

import numpy as np
import pytest
import torch

import mol_likelihood_fixtures as LF
import mol_objective_fixtures as OF
from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4           # the project's relative parity figure (BASELINE.json)
CASES = OF.cases()
SEED = 0x1234ABCD5678EF01


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    g = LF.LLGolden(case)
    batch, sch = g.batch()
    return g, g.model(kind).to(DEV), batch, sch


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _named(model):
    """every name a parameter goes by (tied embeddings and the decoder's aliases included)"""
    return dict(model.named_parameters(remove_duplicate=False))


def _step(model, fn):
    """zero_grad, ``fn() -> loss``, backward -> (loss, {first name: gradient})"""
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _check_grads(got, want32, want64, what):
    """Every tensor within PARITY norm-wise of the fp32 reference gradient, or of the fp64 one where the reference's two runs
    disagree across a ReLU kink; a tensor whose reference gradient is below 1e-6 of the largest: max|got| <= PARITY gmax."""
    gmax = max(np.abs(v).max() for v in want32.values())
    worst = 0.0
    for k, w32 in want32.items():
        a = got[k]
        if np.abs(w32).max() < 1e-6 * gmax:
            assert np.abs(a).max() <= PARITY * gmax, (what, k, np.abs(a).max(), gmax)
            continue
        e = min(rel_err(a, w32), rel_err(a, want64[k]))
        worst = max(worst, e)
        assert e < PARITY, (what, k, e)
    print("%s: %d gradients, largest distance %.3e" % (what, len(want32), worst))


def _reference_parity(name, kind):
    o = OF.ObjGolden(name)
    g, model, batch, sch = _case(o.case, kind)
    eps = torch.from_numpy(o.z["eps"]).to(DEV)
    info = []

    def fn():
        loss, i = model.bound_loss(batch, n_samples=g.K, objective=o.objective, beta=o.beta, mol_weights=o.weights, eps=eps,
                                   schedule=sch)
        info.append(i)
        assert loss.dim() == 0 and loss.requires_grad
        return loss

    loss, grads = _step(model, fn)
    ref = float(o.z["loss"])
    print("%s %s: loss %.9g, reference %.9g" % (name, kind, float(loss), ref))
    assert abs(float(loss) - ref) <= PARITY * abs(ref)
    params = _named(model)
    got = {}
    for k in o.grads(32):
        assert k in params, k
        assert params[k].grad is not None, k
        got[k] = _np(params[k].grad)
    _check_grads(got, {k: v.astype(np.float64) for k, v in o.grads(32).items()},
                 {k: v.astype(np.float64) for k, v in o.grads(64).items()}, "%s %s" % (name, kind))
    # every parameter the reference reaches is reached (asserted above); the property heads and LossWeigh are not
    for k, p in model.named_parameters():
        if k.startswith(("property_optim.", "loss_weigh.")):
            assert p.grad is None, k
    assert info[0].stats == dict(encoder_calls=1, atom_level_calls=1 if g.decoder == "hier" else 0, decoder_passes=g.K)
    want_w = o.weights if o.weights is not None else [1.0] * g.B
    assert np.array_equal(_np(info[0].weights), np.asarray(want_w, np.float32).astype(np.float64))


@pytest.mark.parametrize("name,kind", CASES)
def test_parity_with_the_reference(name, kind):
    _reference_parity(name, kind)


@pytest.mark.parametrize("side", ["0", "1"])
@pytest.mark.parametrize("variant", OF.VARIANTS)
def test_parity_with_the_side_stream_on_and_off(variant, side, monkeypatch):
    """the K entries per parameter of the deferred weight-gradient queue add up with GGPM_SIDE_STREAM on and off"""
    monkeypatch.setenv("GGPM_SIDE_STREAM", side)
    _reference_parity("ll_hier_gru_s40__" + variant, "hier-prop")


@pytest.mark.parametrize("case,kind", [("ll_hier_gru_s40", "hier-prop"), ("ll_hier_lstm_s41", "hier-prop"),
                                       ("ll_motif_gru_s60", "prop"), ("ll_motif_lstm_s61", "prop")])
def test_one_zero_draw_is_the_training_step(case, kind):
    """K = 1, eps = 0, ELBO: the loss and every gradient of ``model(*batch, beta=b, perturb_z=False)`` -- the same addends
    summed in another order"""
    g, model, batch, sch = _case(case, kind)
    b = 0.3
    want_loss, want = _step(model, lambda: model(*batch, beta=b, perturb_z=False, schedule=sch)[0])
    eps = torch.zeros(1, g.B, g.latent, device=DEV)
    got_loss, got = _step(model, lambda: model.bound_loss(batch, n_samples=1, objective="elbo", beta=b, eps=eps, schedule=sch)[0])
    print("%s %s: loss %.9g, training step %.9g" % (case, kind, float(got_loss), float(want_loss)))
    assert abs(float(got_loss) - float(want_loss)) <= PARITY * abs(float(want_loss))
    assert set(got) == set(want)
    w = {k: _np(v) for k, v in want.items()}
    _check_grads({k: _np(v) for k, v in got.items()}, w, w, "%s %s against the training step" % (case, kind))


@pytest.mark.parametrize("case,kind", LF.cases())
def test_info_is_log_likelihoods_and_the_seeded_stream(case, kind):
    g, model, batch, sch = _case(case, kind)
    eps = torch.from_numpy(g.z["eps"]).to(DEV)
    ll = model.log_likelihood(batch, n_samples=g.K, eps=eps, schedule=sch)
    for objective in ("elbo", "iwae"):
        loss, info = model.bound_loss(batch, n_samples=g.K, objective=objective, eps=eps, schedule=sch)
        for what in ("parts", "kl", "elbo", "iwae", "z"):
            a = getattr(info, what)
            assert torch.equal(a, getattr(ll, what)), (objective, what)
            assert not a.requires_grad and a.dtype == torch.float32
        assert info.stats == ll.stats and all(type(v) is int for v in info.stats.values())
        # the loss is the objective of those figures
        terms = -_np(ll.iwae) if objective == "iwae" else _np(ll.parts).sum(axis=2).mean(axis=0) + _np(ll.kl)
        assert abs(float(loss.detach()) - terms.mean()) <= 3 * 2.0 ** -24 * np.abs(terms).mean()     # iwae is stored rounded, the loss once
    # seed=s is the stream's own draws passed as eps=
    from ggpm_amd import functional as F_
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    ids = [7, 3, 11][:g.B]
    draws = F_.sample_latent_normal(2, g.B, g.latent, lo, hi, ids=ids, device=DEV)
    run = lambda **kw: _step(model, lambda: model.bound_loss(batch, n_samples=2, objective="iwae", schedule=sch, **kw)[0])
    a = run(seed=SEED, sample_ids=ids)
    b = run(eps=draws)
    c = run(seed=SEED, sample_ids=ids)
    for (la, ga), (lb, gb) in ((a, b), (a, c)):             # ... and two identical calls are bitwise equal
        assert torch.equal(la, lb) and set(ga) == set(gb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("case,kind", [("ll_hier_lstm_s41", "hier-prop-opt"), ("ll_motif_gru_s60", "prop"),
                                       ("ll_motif_lstm_s61", "prop-opt")])
def test_a_second_step_adds_into_grad(case, kind):
    """no zero_grad between two bound_loss + backward: every .grad is twice the single-pass gradient, to one fp32 rounding
    per element -- tied embedding tables (ll_hier_lstm_s41, ll_motif_lstm_s61), which get one contribution per use,
    included -- and stays the tensor it was"""
    g, model, batch, sch = _case(case, kind)
    fn = lambda: model.bound_loss(batch, n_samples=2, objective="iwae", mol_weights=[0.5, 2.0, 1.25], seed=SEED, schedule=sch)[0]
    _, once = _step(model, fn)
    held = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    fn().backward()
    torch.cuda.synchronize()
    bad = []
    for k, p in model.named_parameters():
        if k in once:
            assert p.grad is held[k], k
            a, w = _np(p.grad), 2 * _np(once[k])
            r = float((np.abs(a - w) / np.maximum(2.0 ** -24 * np.abs(w), 1e-300)).max())
            print("%s %s %s: largest distance %.2f roundings" % (case, kind, k, r))
            if r > 1.0:
                bad.append((k, r))
    model.zero_grad(set_to_none=True)
    assert not bad, bad


def test_a_step_on_other_gradients_adds_to_them():
    """.grad holding something else (here: a training step's gradient): bound_loss + backward adds its own gradient to it,
    one rounding per element"""
    g, model, batch, sch = _case("ll_hier_lstm_s41", "hier-prop")
    fn = lambda: model.bound_loss(batch, n_samples=2, seed=SEED, schedule=sch)[0]
    _, own = _step(model, fn)
    _, other = _step(model, lambda: model(*batch, beta=0.1, perturb_z=False, schedule=sch)[0])
    fn().backward()
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        if k in own:
            w = _np(own[k]) + _np(other[k])
            assert (np.abs(_np(p.grad) - w) <= 2.0 ** -24 * np.abs(w)).all(), k
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("case,kind", [("ll_hier_gru_s40", "hier-prop"), ("ll_motif_lstm_s61", "prop-opt")])
def test_second_backward_raises(case, kind):
    g, model, batch, sch = _case(case, kind)
    model.zero_grad(set_to_none=True)
    loss, _ = model.bound_loss(batch, n_samples=2, seed=SEED, schedule=sch)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a retained graph is not supported"):
        loss.backward()
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)


def test_pinned_max_cls_size_moves_the_attachment_gradient_only_through_its_rows():
    """max_cls_size above the batch's own: info equals log_likelihood's with the same pin, and the gradients stay finite and
    within the parity figure of the unpinned ones plus what the extra zero candidates add (checked through the loss:
    finite differences would need a second reference)"""
    g, model, batch, sch = _case("ll_hier_gru_s40", "hier-prop")
    eps = torch.from_numpy(g.z["eps"]).to(DEV)
    C = sch.max_cls_size + 4
    ll = model.log_likelihood(batch, n_samples=g.K, eps=eps, schedule=sch, max_cls_size=C)
    info = []

    def fn():
        loss, i = model.bound_loss(batch, n_samples=g.K, eps=eps, schedule=sch, max_cls_size=C)
        info.append(i)
        return loss

    loss, grads = _step(model, fn)
    assert torch.equal(info[0].parts, ll.parts)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    # W_assm.bias: every candidate of a prediction shares it, so its gradient stays analytically zero with the pad rows too
    gmax = max(float(v.abs().max()) for v in grads.values())
    assert float(grads["decoder.W_assm.bias"].abs().max()) <= PARITY * gmax
    model.zero_grad(set_to_none=True)


def test_argument_errors():
    g, model, batch, sch = _case("ll_hier_gru_s40", "hier-prop")
    with pytest.raises(ValueError, match="beta"):
        model.bound_loss(batch, objective="iwae", beta=0.5, schedule=sch)
    with pytest.raises(ValueError, match="mol_weights"):
        model.bound_loss(batch, mol_weights=[1.0, 2.0], schedule=sch)
    with pytest.raises(ValueError, match="mol_weights"):
        model.bound_loss(batch, mol_weights=torch.ones(g.B + 1, device=DEV), schedule=sch)
    with pytest.raises(ValueError, match="objective"):
        model.bound_loss(batch, objective="vae", schedule=sch)
    with pytest.raises(ValueError, match=r"bound_loss: n_samples"):
        model.bound_loss(batch, n_samples=0, schedule=sch)
    with pytest.raises(ValueError, match=r"bound_loss: eps of shape"):
        model.bound_loss(batch, n_samples=2, eps=torch.zeros(1, g.B, g.latent, device=DEV), schedule=sch)
    m2 = g.model("hier-prop", dropout=0.1).to(DEV)
    m2.train()
    with pytest.raises(NotImplementedError, match=r"bound_loss runs without dropout: call model\.eval\(\) first"):
        m2.bound_loss(batch, schedule=sch)
    # a tensor of weights on the device is taken as it is; without backward nothing gains a .grad
    model.zero_grad(set_to_none=True)
    loss, info = model.bound_loss(batch, mol_weights=torch.tensor([0.5, 2.0, 1.25], device=DEV), seed=SEED, schedule=sch)
    assert torch.equal(info.weights, torch.tensor([0.5, 2.0, 1.25], device=DEV)) and all(p.grad is None for p in model.parameters())
