"""GPU: PropertyVAEOptimizer.search / search_and_decode on the small HierPropOptVAE and PropOptVAE fixture models, against
tests/latent_search_oracle.py run on the model's own posterior and starts.  Bound as in
tests/test_latent_search_kernels_gpu.py: max(1e-4, 4 |oracle fp32 - oracle fp64|) per element, step counts exactly."""
import functools

import numpy as np
import pytest
import torch

import latent_search_oracle as lso
import property_oracle as po
from decode_fixtures import norm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["hier", "motif"]
SEED = 0x5EA2C4D00D15EA5E
K, STEPS, LR, MOM, AW, PW = 3, 10, 0.02, 0.9, 0.3, 0.1


class _Args:
    optimize_type, property_optim_step, patience, patience_threshold = "fixed", STEPS, 3, 0.01
    property_delta, latent_lr, max_steps = 0.01, LR, 10000

    def __init__(self, factory):
        self.graph_batch_factory = factory


def _make(kind):
    """a fresh (model in eval mode, batch, schedule, specs, the kind's synthetic graph batch, the fixture)"""
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.synth_graph import SynthAtomVocab, SynthGraphBatch, SynthHierGraphBatch
    if kind == "hier":
        import property_fixtures as pf
        from ggpm_amd.property_vae import HierPropOptVAE
        from ggpm_amd.vocab import IndexPairVocab
        g = pf.PropOptGolden(pf.names("propopt")[0])
        args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
        args.atom_vocab = SynthAtomVocab()
        model = HierPropOptVAE(args).to(DEV)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=False)
        specs = g.specs()
        tensors = synth.tensorize(specs)
        batch = (None, None, tensors, [None] * g.B, g.z["t_homo"].tolist(), g.z["t_lumo"].tolist())
        return model.eval(), batch, DecodeSchedule.from_specs(specs, tensors), specs, SynthHierGraphBatch, g
    from motif_fixtures import MotifGolden
    g = MotifGolden("propopt_gru_s63")
    tensors, sch, orders, homos, lumos = g.batch()
    return g.model().to(DEV).eval(), (None, None, tensors, orders, homos, lumos), sch, g.specs(), SynthGraphBatch, g


@functools.lru_cache(maxsize=None)
def _case(kind):
    from ggpm_amd.property_control import HierPropertyVAEOptimizer, PropertyVAEOptimizer
    model, batch, sch, specs, factory, g = _make(kind)
    cls = HierPropertyVAEOptimizer if kind == "hier" else PropertyVAEOptimizer
    return model, cls(model, _Args(factory)), batch, sch, specs


def _np(t):
    return t.detach().cpu().numpy()


def _prior(L, C=4):
    from ggpm_amd.prior import MixturePrior
    torch.manual_seed(7)
    return MixturePrior(C, L, init_std=0.7).to(DEV)


@functools.lru_cache(maxsize=None)
def _posterior(kind):
    """the model's own mu, lv [B, L] and the K starts of SEED (numpy fp32), the heads' layers"""
    from ggpm_amd.latent_heads import _encode_heads
    from ggpm_amd.nnutils import make_cuda
    model, search, batch, sch, _ = _case(kind)
    with torch.no_grad():
        _, mu, pre_var = _encode_heads(model, make_cuda(batch[2]))
    z = model.log_likelihood(batch, n_samples=K, seed=SEED, schedule=sch).z.clone()
    z[0] = mu
    sd = {k: _np(v) for k, v in model.state_dict().items()}
    layers = tuple(po.head_layers(sd, "property_optim." + h, np.float32) for h in ("homo_linear", "lumo_linear"))
    return _np(mu), -np.abs(_np(pre_var)), _np(z), layers


def _oracle(kind, starts, steps, momentum, aw, pw, prior, delta=-1.0, weights=(1.0, 1.0)):
    mu, lv, z, (homo, lumo) = _posterior(kind)
    _, _, batch, _, _ = _case(kind)
    B, L = mu.shape
    pr = None if prior is None else tuple(_np(p) for p in (prior.logits, prior.means, prior.log_vars))
    runs, margins = [], []
    for dt in (np.float32, np.float64):
        m = lso.Margins()
        runs.append(lso.search(homo, lumo, z[:starts].reshape(starts * B, L), L // 2, mu, lv, batch[4], batch[5], starts, B, LR,
                               momentum, steps, delta, weights[0], weights[1], aw, pw, prior=pr, dtype=dt, margins=m))
        margins.append(m)
    return runs[0], runs[1], margins


def _within(what, got, r32, r64):
    bound = np.maximum(1e-4, 4 * np.abs(r32.astype(np.float64) - r64))
    err = np.abs(_np(got).astype(np.float64) - r32.astype(np.float64))
    print("%s: worst error %.3e, worst error / bound %.3f" % (what, err.max(), (err / bound).max()))
    assert (err <= bound).all(), "%s: worst excess %.3e" % (what, (err - bound).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mixture", [False, True])
def test_search_matches_the_oracle_on_the_models_own_posterior_and_starts(kind, mixture):
    model, search, batch, sch, _ = _case(kind)
    B, L = len(batch[4]), 2 * model.latent_size
    prior = _prior(L) if mixture else None
    res = search.search(batch, n_starts=K, momentum=MOM, anchor_weight=AW, prior_weight=PW, prior=prior, seed=SEED,
                        weights=(1.0, 0.5))
    r32, r64, (m32, m64) = _oracle(kind, K, STEPS, MOM, AW, PW, prior, weights=(1.0, 0.5))
    print("%s: smallest decision margin of the fp64 run %s" % (kind, m64.by_kind))
    assert m32.same_decisions(m64)
    assert res.all_latents.shape == (K, B, L) and res.latent.shape == (B, L) and res.terms.shape == (B, 3)
    for t in (res.latent, res.terms, res.all_latents, res.all_objectives, res.all_terms) + tuple(res.predictions):
        assert t.dtype == torch.float32 and t.device == torch.device(DEV) and not t.requires_grad
    assert res.best_start.dtype == torch.int32 and res.steps_taken.dtype == torch.int32
    assert (_np(res.steps_taken).reshape(-1) == r32["steps"]).all()
    _within("all_latents", res.all_latents.reshape(K * B, L), r32["z"], r64["z"])
    _within("all_objectives", res.all_objectives.reshape(-1), r32["J"], r64["J"])
    _within("all_terms", res.all_terms.reshape(K * B, 3), r32["terms"], r64["terms"])
    best = r32["best"]
    assert _np(res.best_start).tolist() == best.tolist() and (r64["best"] == best).all()
    rows = best * B + np.arange(B)
    _within("latent", res.latent, r32["z"][rows], r64["z"][rows])
    _within("terms", res.terms, r32["terms"][rows], r64["terms"][rows])
    _within("predictions", torch.stack(res.predictions), r32["pred"][:, rows], r64["pred"][:, rows])
    # the selected row is the row: bit for bit what the search left at best_start
    pick = res.best_start.long()
    assert torch.equal(res.latent, res.all_latents[pick, torch.arange(B, device=DEV)])
    assert torch.equal(res.terms, res.all_terms[pick, torch.arange(B, device=DEV)])


@pytest.mark.parametrize("kind", KINDS)
def test_start_k_is_draw_k_of_log_likelihood_and_start_0_the_posterior_mean(kind):
    model, search, batch, sch, _ = _case(kind)
    mu, _, z, _ = _posterior(kind)
    res = search.search(batch, n_starts=K, steps=0, seed=SEED)
    assert (_np(res.steps_taken) == 0).all()
    assert (_np(res.all_latents)[0] == mu).all()
    assert (_np(res.all_latents)[1:] == z[1:]).all() and not (z[1] == z[2]).all()
    five = search.search(batch, n_starts=5, steps=0, seed=SEED)
    assert torch.equal(five.all_latents[:K], res.all_latents)                 # the prefix property of the draws
    other = search.search(batch, n_starts=K, steps=0, seed=SEED + 1)
    assert torch.equal(other.all_latents[0], res.all_latents[0]) and not torch.equal(other.all_latents[1], res.all_latents[1])
    torch.manual_seed(3)
    a = search.search(batch, n_starts=2, steps=0)                             # seed=None: torch's default CPU generator
    torch.manual_seed(3)
    b = search.search(batch, n_starts=2, steps=0)
    assert torch.equal(a.all_latents, b.all_latents)


@pytest.mark.parametrize("kind", KINDS)
def test_one_start_without_regularisers_is_plain_descent_from_the_mean(kind):
    model, search, batch, sch, _ = _case(kind)
    res = search.search(batch, momentum=0.0)
    r32, r64, _ = _oracle(kind, 1, STEPS, 0.0, 0.0, 0.0, None)
    assert (_np(res.best_start) == 0).all() and (_np(res.steps_taken) == STEPS).all()
    _within("latent", res.latent, r32["z"], r64["z"])
    _within("predictions", torch.stack(res.predictions), r32["pred"], r64["pred"])
    assert torch.equal(res.latent, res.all_latents[0]) and torch.equal(res.all_objectives[0], res.terms[:, 0])
    half = model.latent_size
    with torch.no_grad():
        again = model.property_optim.predict(homo_vecs=res.latent[:, :half], lumo_vecs=res.latent[:, half:])
    _within("predict(latent)", torch.stack(again), _np(torch.stack(res.predictions)), _np(torch.stack(res.predictions)).astype(np.float64))


@pytest.mark.parametrize("kind", KINDS)
def test_a_positive_anchor_weight_keeps_the_selected_latent_nearer_the_posterior(kind):
    model, search, batch, sch, _ = _case(kind)
    free = search.search(batch, n_starts=K, steps=25, lr=0.05, anchor_weight=0.0, seed=SEED)
    held = search.search(batch, n_starts=K, steps=25, lr=0.05, anchor_weight=0.5, seed=SEED)
    print(kind, "anchor term, free:", _np(free.terms[:, 1]), "held:", _np(held.terms[:, 1]))
    assert bool((held.terms[:, 1] < free.terms[:, 1]).all())


@pytest.mark.parametrize("kind", KINDS)
def test_a_molecules_starts_follow_its_sample_id_not_its_batch(kind):
    """alone in a batch under its own sample id a molecule gets the starts it gets inside the batch (the encoder's row tiles
    differ between the two batches, so mu and lv agree at the parity figure and not bit for bit); under another id it does not"""
    from ggpm_amd import synth
    from ggpm_amd.decoder import synth_orders
    model, search, batch, sch, specs = _case(kind)
    B = len(batch[4])
    ids = [100 + 7 * b for b in range(B)]
    full = _np(search.search(batch, n_starts=K, steps=0, seed=SEED, sample_ids=ids).all_latents)
    i = B - 1
    tensors = synth.tensorize(specs[i:i + 1])
    orders = synth_orders(specs[i:i + 1], tensors[0][-1]) if kind == "motif" else [None]
    one = (None, None, tensors, orders, batch[4][i:i + 1], batch[5][i:i + 1])
    alone = _np(search.search(one, n_starts=K, steps=0, seed=SEED, sample_ids=[ids[i]]).all_latents)[:, 0]
    scale = np.abs(full[:, i]).max()
    assert np.abs(alone - full[:, i]).max() <= 1e-4 * scale
    wrong = _np(search.search(one, n_starts=K, steps=0, seed=SEED, sample_ids=[ids[i] + 1]).all_latents)[:, 0]
    assert np.abs(wrong[1:] - full[1:, i]).max() > 1e-2 * scale
    reordered = _np(search.search(batch, n_starts=K, steps=0, seed=SEED, sample_ids=ids[::-1]).all_latents)
    assert not (reordered[1:] == full[1:]).all() and (reordered[0] == full[0]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_grads_rng_state_and_the_next_training_step_are_untouched(kind):
    model, batch, sch, _, _, _ = _make(kind)
    fresh = _make(kind)[0]
    from ggpm_amd.property_control import PropertyVAEOptimizer

    def step(m):
        m.zero_grad(set_to_none=True)
        loss = m(*batch, beta=0.1, perturb_z=False, schedule=sch)[0]
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    step(fresh)
    want_loss, want = step(fresh)
    step(model)
    marker = {k: torch.full_like(p, 3.0) for k, p in model.named_parameters()}
    for k, p in model.named_parameters():
        p.grad = marker[k].clone()
    prior = _prior(2 * model.latent_size)
    search = PropertyVAEOptimizer(model, _Args(None))
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    keys = set(vars(model)) | set(vars(model.decoder)) | set(vars(model.property_optim))
    search.search(batch, n_starts=K, anchor_weight=AW, prior_weight=PW, prior=prior, seed=SEED)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, marker[k]), k
    assert set(vars(model)) | set(vars(model.decoder)) | set(vars(model.property_optim)) == keys
    assert search.steps_taken is None and search.status is None
    got_loss, got = step(model)
    assert torch.equal(got_loss, want_loss) and set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("kind", KINDS)
def test_search_and_decode_decodes_the_selected_latent(kind):
    model, search, batch, sch, _ = _case(kind)
    from ggpm_amd.synth_graph import SynthGraphBatch, SynthHierGraphBatch
    factory = SynthHierGraphBatch if kind == "hier" else SynthGraphBatch
    kw = dict(n_starts=K, momentum=MOM, anchor_weight=AW, prior_weight=PW, seed=SEED)
    props, decoded = search.search_and_decode(batch, _Args(factory), **kw)
    res = search.search(batch, **kw)
    z = res.latent
    want = model.decoder.decode(batch[0], (z, z, z), greedy=True, max_decode_step=150, graph_batch_factory=factory)
    assert norm(decoded) == norm(want)
    for a, b in zip(props, res.predictions):
        assert torch.equal(a, b)
    model.decoder.graph_batch_factory = None
    with pytest.raises(NotImplementedError):
        search.search_and_decode(batch, None, **kw)
    model.decoder.graph_batch_factory = factory            # the decoder's factory when args names none
    try:
        assert norm(search.search_and_decode(batch, None, **kw)[1]) == norm(want)
    finally:
        model.decoder.graph_batch_factory = None


def test_refusals():
    from ggpm_amd.prior import MixturePrior
    model, search, batch, sch, _ = _case("hier")
    B, L = len(batch[4]), 2 * model.latent_size
    for bad in (0, 1025, 1.5, True):
        with pytest.raises(ValueError, match="n_starts"):
            search.search(batch, n_starts=bad)
    with pytest.raises(ValueError, match="sample_ids"):
        search.search(batch, n_starts=2, sample_ids=list(range(B + 1)))
    for kw in (dict(anchor_weight=-0.1), dict(prior_weight=-1.0), dict(weights=(1.0, -1.0)), dict(momentum=-0.5),
               dict(steps=-1), dict(anchor_weight=float("nan"))):
        with pytest.raises(ValueError, match="finite value >= 0"):
            search.search(batch, **kw)
    with pytest.raises(ValueError, match="MixturePrior"):
        search.search(batch, prior=torch.zeros(3))
    with pytest.raises(ValueError, match="latent columns"):
        search.search(batch, prior=MixturePrior(2, L + 2).to(DEV))
    with pytest.raises(ValueError, match="the prior is on"):
        search.search(batch, prior=MixturePrior(2, L))
    model.property_optim.train()
    drops = [m for m in model.property_optim.modules() if isinstance(m, torch.nn.Dropout)]
    saved = [m.p for m in drops]
    try:
        for m in drops:
            m.p = 0.1
        with pytest.raises(RuntimeError, match="eval"):
            search.search(batch)
    finally:
        for m, p in zip(drops, saved):
            m.p = p
        model.property_optim.eval()
