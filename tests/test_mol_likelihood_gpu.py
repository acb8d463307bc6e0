"""GPU: ``log_likelihood`` of the four VAEs end to end -- against the reference's per-molecule figures (the fixtures of
tests/golden/make_golden_mol_likelihood.py, ``eps=`` given), against the training forward of the same model, across batch
compositions, across seeds, for what it issues (``stats``) and for what it leaves behind (nothing)."""
import functools

import numpy as np
import pytest
import torch

import mol_likelihood_fixtures as LF
from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4           # the project's relative parity figure (BASELINE.json)
CASES = LF.cases()
SEED = 0x1234ABCD5678EF01


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    g = LF.LLGolden(name)
    batch, sch = g.batch()
    return g, g.model(kind).to(DEV), batch, sch


@functools.lru_cache(maxsize=None)
def _fixture_run(name, kind):
    """The fixture's K = 3 recorded draws through the model: computed once, shared, left unchanged."""
    g, model, batch, sch = _case(name, kind)
    out = model.log_likelihood(batch, n_samples=g.K, eps=torch.from_numpy(g.z["eps"]).to(DEV), schedule=sch)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name,kind", CASES)
def test_fixture_parity(name, kind):
    g, model, batch, sch = _case(name, kind)
    out = _fixture_run(name, kind)
    z = g.z
    K, B, L = g.K, g.B, g.latent
    assert out.parts.shape == (K, B, 4) and out.kl.shape == (B,) and out.elbo.shape == (B,) and out.iwae.shape == (B,)
    assert out.z.shape == (K, B, L)
    for t in (out.parts, out.kl, out.elbo, out.iwae, out.z):
        assert t.dtype == torch.float32 and t.device == DEV and not t.requires_grad
    parts = _np(out.parts)
    for t, what in enumerate(("topo", "cls", "icls", "assm")):
        e = rel_err(parts[:, :, t], z["parts"][:, :, t])
        print("%s %s parts[%s]: %.3e" % (name, kind, what, e))
        assert e < PARITY, (what, e)
    assert ((parts[:, :, 3] == 0) == (z["parts"][:, :, 3] == 0)).all()           # molecules without attachment predictions
    for got, what in ((out.kl, "kl"), (out.elbo, "elbo"), (out.iwae, "iwae")):
        e = rel_err(_np(got), z[what])
        print("%s %s %s: %.3e" % (name, kind, what, e))
        assert e < PARITY, (what, e)
    lv = -np.abs(z["pre_var"].astype(np.float64))
    assert rel_err(_np(out.z), z["mean"][None] + np.exp(lv / 2)[None] * z["eps"]) < PARITY


def _forward(model, batch, sch, kind):
    """(reconstruction loss, KL) of the existing no-grad forward with perturb_z=False.  beta = 0 makes `loss - beta KL` exact."""
    with torch.no_grad():
        out = model(*batch, beta=0.0, perturb_z=False, schedule=sch)
    m = out[1]
    if kind.endswith("-opt"):
        return float(m["Recs_Loss"]), float(m["KL"])
    return float(m["Loss"]), float(m["KL:"])


@pytest.mark.parametrize("name,kind", CASES)
def test_zero_eps_is_the_training_loss_and_kl(name, kind):
    """eps = 0, K = 1: the same rows as the forward's, summed in another order; all addends have one sign, so the two sums
    differ by at most n_addends 2^-24 relative"""
    g, model, batch, sch = _case(name, kind)
    B, L = g.B, g.latent
    out = model.log_likelihood(batch, n_samples=1, eps=torch.zeros(1, B, L, device=DEV), schedule=sch)
    loss, kl = _forward(model, batch, sch, kind)
    n_rows = len(sch.topo()[0]) + 2 * len(sch.cls()[0]) + len(sch.assm_batch())
    got = float(_np(out.parts).sum()) / B
    print("%s %s: loss %.9g vs %.9g (%d rows), KL %.9g vs %.9g" % (name, kind, got, loss, n_rows, float(_np(out.kl).sum()) / B, kl))
    assert abs(got - loss) <= n_rows * 2.0 ** -24 * abs(loss), (got, loss)
    got_kl = float(_np(out.kl).sum()) / B
    assert abs(got_kl - kl) <= B * L * 2.0 ** -24 * abs(kl), (got_kl, kl)
    # K = 1: the bound is the single-sample ELBO estimate; with eps = 0, log p(z) - log q(z | x) = -0.5 sum z^2 + 0.5 sum lv
    nll = _np(out.parts)[0].sum(axis=1)
    assert rel_err(_np(out.iwae), -nll + 0.5 * (-np.abs(g.z["pre_var"].astype(np.float64))).sum(axis=1)
                   - 0.5 * (_np(out.z)[0] ** 2).sum(axis=1)) < PARITY


@pytest.mark.parametrize("name,kind", CASES)
def test_same_seed_twice_is_bitwise_equal_and_stats_count_the_passes(name, kind):
    g, model, batch, sch = _case(name, kind)
    a = model.log_likelihood(batch, n_samples=3, seed=SEED, schedule=sch)
    b = model.log_likelihood(batch, n_samples=3, seed=SEED, schedule=sch)
    for what in ("parts", "kl", "elbo", "iwae", "z"):
        assert torch.equal(getattr(a, what), getattr(b, what)), what
    c = model.log_likelihood(batch, n_samples=3, seed=SEED + 1, schedule=sch)
    assert not torch.equal(c.z, a.z)
    assert torch.equal(c.kl, a.kl)                      # the KL is analytic: no draw enters it
    five = model.log_likelihood(batch, n_samples=5, seed=SEED, schedule=sch)
    assert torch.equal(five.z[:3], a.z) and torch.equal(five.parts[:3], a.parts)        # the prefix property, end to end
    want = dict(encoder_calls=1, atom_level_calls=1 if g.decoder == "hier" else 0, decoder_passes=3)
    assert a.stats == want and all(type(v) is int for v in a.stats.values())
    assert five.stats == dict(want, decoder_passes=5)
    torch.manual_seed(11)
    d = model.log_likelihood(batch, n_samples=2, schedule=sch)      # seed=None: torch's default CPU generator
    torch.manual_seed(11)
    e = model.log_likelihood(batch, n_samples=2, schedule=sch)
    assert torch.equal(d.z, e.z)


@pytest.mark.parametrize("name,kind", CASES)
def test_nothing_is_left_behind(name, kind):
    """no parameter gains a .grad, and a training step after the call equals the same step on a fresh model bit for bit"""
    g = LF.LLGolden(name)
    batch, sch = g.batch()

    def step(model):
        model.zero_grad(set_to_none=True)
        loss = model(*batch, beta=0.1, perturb_z=False, schedule=sch)[0]
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    fresh = g.model(kind).to(DEV)
    step(fresh)
    want_loss, want = step(fresh)
    model = g.model(kind).to(DEV)
    step(model)
    model.zero_grad(set_to_none=True)
    model.log_likelihood(batch, n_samples=2, seed=SEED, schedule=sch)
    assert all(p.grad is None for p in model.parameters())
    assert not hasattr(model.decoder, "_atom_ahead") and not hasattr(model.decoder, "_heads_in")
    got_loss, got = step(model)
    assert torch.equal(got_loss, want_loss)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("name,kind", [("ll_hier_gru_s40", "hier-prop"), ("ll_hier_lstm_s41", "hier-prop-opt"),
                                       ("ll_motif_lstm_s61", "prop")])
def test_stats_are_what_the_call_issues(name, kind, monkeypatch):
    """the structural claim, counted where the work is issued: the encoder and the decoder's atom level run once whatever
    K is, the tree-side levels and the heads K times"""
    from ggpm_amd import heads_fused, motif_decoder, tree_decode
    g, model, batch, sch = _case(name, kind)
    calls = dict(encoder=0, atom=0, tree=0, heads=0)

    def counted(what, fn):
        def wrapper(*a, **kw):
            calls[what] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(model.encoder, "forward_padded", counted("encoder", model.encoder.forward_padded))
    monkeypatch.setattr(tree_decode, "_tree_level_infer", counted("tree", tree_decode._tree_level_infer))
    hier = g.decoder == "hier"
    if hier:
        monkeypatch.setattr(model.decoder, "_atom_level", counted("atom", model.decoder._atom_level))
        monkeypatch.setattr(heads_fused, "_heads_forward", counted("heads", heads_fused._heads_forward))
    else:
        monkeypatch.setattr(motif_decoder, "bce_rows", counted("heads", motif_decoder.bce_rows))
    K = 3
    out = model.log_likelihood(batch, n_samples=K, seed=SEED, schedule=sch)
    assert calls == dict(encoder=1, atom=1 if hier else 0, tree=(2 if hier else 1) * K, heads=K), calls
    assert out.stats == dict(encoder_calls=calls["encoder"], atom_level_calls=calls["atom"], decoder_passes=calls["heads"])


def test_training_mode_with_dropout_raises():
    g = LF.LLGolden("ll_hier_gru_s40")
    batch, sch = g.batch()
    model = g.model("hier-prop", dropout=0.1).to(DEV)
    model.train()
    with pytest.raises(NotImplementedError, match=r"log_likelihood runs without dropout: call model\.eval\(\) first"):
        model.log_likelihood(batch, schedule=sch)
    model.eval()
    assert model.log_likelihood(batch, schedule=sch).stats["decoder_passes"] == 1


@pytest.mark.parametrize("name", ["ll_hier_lstm_s41", "ll_motif_lstm_s61"])
def test_decoder_molecule_losses_is_the_per_molecule_form_of_forward(name):
    """the decoder-level entry on given latents: [B, 4], summing to forward's loss x B"""
    kind = "hier-prop" if name.startswith("ll_hier") else "prop"
    g, model, batch, sch = _case(name, kind)
    from ggpm_amd.nnutils import make_cuda
    z = torch.from_numpy(g.z["mean"]).to(DEV)
    tensors = make_cuda(batch[2])
    with torch.no_grad():
        loss = model.decoder(None, (z, z, z), None, tensors, batch[3], schedule=sch)[0]
    parts = model.decoder.molecule_losses(None, (z, z, z), None, tensors, batch[3], schedule=sch)
    assert parts.shape == (g.B, 4) and not parts.requires_grad
    n_rows = len(sch.topo()[0]) + 2 * len(sch.cls()[0]) + len(sch.assm_batch())
    assert abs(float(_np(parts).sum()) / g.B - float(loss)) <= n_rows * 2.0 ** -24 * abs(float(loss))


# (last: the only test on a batch shape -- one molecule -- no other GPU test of these models runs)
@pytest.mark.parametrize("name,kind", [c for c in CASES if c[1] in ("hier-prop", "prop")])
def test_a_molecule_alone_gets_its_numbers(name, kind):
    """max_cls_size pinned to the full batch's and the molecule's own sample id: the same eps bit for bit, and -- the GEMM row
    tiles differ -- the same parts / kl / iwae at the parity figure"""
    from ggpm_amd import functional as F_, synth
    from ggpm_amd.decoder import DecodeSchedule, synth_orders
    g, model, batch, sch = _case(name, kind)
    K, L = 3, g.latent
    full = model.log_likelihood(batch, n_samples=K, seed=SEED, schedule=sch)
    specs = g.specs()
    i = max(range(g.B), key=lambda j: specs[j].n_motifs)
    tensors = synth.tensorize(specs[i:i + 1])
    orders = synth_orders(specs[i:i + 1], tensors[0][-1]) if g.decoder == "motif" else [None]
    sch1 = DecodeSchedule.from_specs(specs[i:i + 1], tensors)
    one = model.log_likelihood((None, None, tensors, orders, [0.0], [0.0]), n_samples=K, seed=SEED, sample_ids=[i],
                               max_cls_size=sch.max_cls_size, schedule=sch1)
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    eps_full = F_.sample_latent_normal(K, g.B, L, lo, hi, device=DEV)
    eps_one = F_.sample_latent_normal(K, 1, L, lo, hi, ids=[i], device=DEV)
    assert torch.equal(eps_one[:, 0], eps_full[:, i])
    for what in ("parts", "kl", "iwae", "elbo", "z"):
        a, b = _np(getattr(one, what)), _np(getattr(full, what))
        b = b[:, i:i + 1] if b.ndim > 1 else b[i:i + 1]
        e = rel_err(a, b)
        print("%s %s molecule %d alone, %s: %.3e" % (name, kind, i, what, e))
        assert e < PARITY, (what, e)
    with pytest.raises(ValueError, match="max_cls_size"):
        model.log_likelihood(batch, schedule=sch, max_cls_size=sch.max_cls_size - 2)
    # a larger pinned size adds zero candidates, which score b_assm . z: the attachment term moves, the others do not
    wide = model.log_likelihood(batch, n_samples=K, seed=SEED, schedule=sch, max_cls_size=sch.max_cls_size + 4)
    assert torch.equal(wide.parts[:, :, :3], full.parts[:, :, :3])
    has = _np(full.parts)[:, :, 3] > 0
    assert (_np(wide.parts)[:, :, 3][has] >= _np(full.parts)[:, :, 3][has]).all()
    assert (_np(wide.parts)[:, :, 3][has] > _np(full.parts)[:, :, 3][has]).any()
    assert (_np(wide.parts)[:, :, 3][~has] == 0).all()
