"""CPU: the sampled mode of the decode loop (``decode_sampled``) on the fp64 restatements of the kernels -- the reference's
own ``decode(greedy=False)`` replayed draw for draw (tests/golden/*_decode_sampled), the properties of the seeded stream
on the restated sampler (tests/sample_oracle.py), and the entry points."""
import numpy as np
import pytest
import torch

import sample_oracle as SO
import sampled_decode_fixtures as SF
from decode_fixtures import assert_same, norm
from ggpm_amd import greedy_decode as G

CASES = SF.cases()
IDS = [kind + "-" + name for kind, name in CASES]


def test_the_fixtures_are_two_per_decoder_and_exercise_the_draws():
    assert sorted(k for k, _ in CASES) == ["hier", "hier", "motif", "motif"]
    for kind in ("motif", "hier"):
        assert {SF.load(k, n).rnn for k, n in CASES if k == kind} == {"GRU", "LSTM"}
    for kind, name in CASES:
        g = SF.load(kind, name)
        assert (g.H, g.B) == (16, 4) and g.max_step <= 30 and float(g.z["margin"]) >= 1e-4
        assert any((p > 0.5) != (d > 0.5) for ps, ds in g.bernoulli for p, d in zip(ps, ds))
        assert any(row != sorted(row) for _, rows in g.multinomial for row in rows)
        assert any("Attaching Fragment" in e and e["Attaching Fragment"][0] != e["top-5-inter-cands"][0][1]
                   for r in g.results for e in r[1:])


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_replaying_the_reference_draws_reproduces_its_sampled_decode(kind, name):
    g = SF.load(kind, name)
    d, replay = g.decoder(), g.replay()
    made = []

    def factory(*a, **k):
        made.append(SF.graph_batch(kind)(*a, **k))
        return made[-1]
    results, mols = SF.module(kind).decode_sampled(d, None, g.latents("cpu"), max_decode_step=g.max_step, beam=g.beam,
                                                   graph_batch_factory=factory, backend=SF.oracle_backend(kind),
                                                   sampler=replay)
    assert replay.exhausted()
    if kind == "hier":
        g.check(d, results, mols, made[0])
    else:
        g.check(d, results, mols)
    draws = [e["Generate fragment"] for r in norm(results) for e in r[1:] if "Generate fragment" in e]
    assert set(draws) == {0.0, 1.0}                 # the entry records the draw, not the probability
    tried = [kk for _, _, kk, _, _ in d.last_decode_trace]
    assert any(b < a for a, b in zip(tried, tried[1:]))     # the trace keeps an entry's place in the top k


class DrawingOracle:
    """an oracle backend that draws for itself from the restated stream, the way the device backend does: the loop hands
    it the seed and the ids (``start_sampling``) and the step, and reads ``topo_draws`` / ``beam_order``"""

    @staticmethod
    def of(kind):
        base = SF.oracle_backend(kind)

        class Backend(base):
            def start_sampling(self, sampling):
                self.seed = sampling.seed_lo | sampling.seed_hi << 32
                self.ids = sampling.ids

            def phase1(self, tedits, aedits, edges, atoms, nodes, bidx):
                p = base.phase1(self, tedits, aedits, edges, atoms, nodes, bidx)
                self.topo_draws = SO.topo_draws(self.seed, self.ids[list(bidx)], self.step, p)
                return p

            def phase2(self, tedits, nodes, mess, expanding, k):
                top = base.phase2(self, tedits, nodes, mess, expanding, k)
                if top is not None:
                    self.beam_order = SO.beam_order(self.seed, self.ids[list(expanding)], self.step, top[0])[0]
                return top
        return Backend


def _sampled(g, seed, rows=None, sample_ids=None, backend=None, d=None):
    sampler = None if backend is not None else SO.Sampler(seed)
    d = g.decoder() if d is None else d
    out = SF.decode_sampled(g, d, g.latents("cpu"), rows, seed=seed, sample_ids=sample_ids,
                            backend=backend or SF.oracle_backend(g.kind), sampler=sampler)
    return out, sampler


@pytest.mark.parametrize("kind,name", CASES[::2], ids=IDS[::2])
def test_stream_properties(kind, name):
    g = SF.load(kind, name)
    ids = [10, 11, 12, 13]
    (r1, m1), s1 = _sampled(g, SF.SEED, sample_ids=ids)
    (r2, m2), _ = _sampled(g, SF.SEED, sample_ids=ids)
    assert norm(r1) == norm(r2) and m1 == m2                        # the same seed: the same decode
    assert s1.n_topo > g.B and s1.n_order > 0
    (r3, m3), _ = _sampled(g, SF.SEED + 1, sample_ids=ids)
    assert any(SF.own(a) != SF.own(b) for a, b in zip(r1, r3))      # another seed: another decode
    # molecules 1 and 3 alone, under their own ids: what they were inside the batch of four
    (rs, ms), _ = _sampled(g, SF.SEED, rows=[1, 3], sample_ids=[11, 13])
    for j, b in enumerate((1, 3)):
        assert_same(SF.own(rs[j]), SF.own(r1[b]), path="molecule %d" % b)
        assert ms[j] == m1[b]
    # the draws the backend makes for itself are the sampler's
    (r4, m4), _ = _sampled(g, SF.SEED, sample_ids=ids, backend=DrawingOracle.of(kind))
    assert norm(r4) == norm(r1) and m4 == m1


def test_the_restated_sampler_ranks_masked_entries_by_their_scores():
    """the seam hands ``order`` the probabilities and the scores: masked entries, whose probabilities are all 0, are
    ranked by their keys as the device ranks them, not in index order"""
    import sample_kernel_inputs as KI
    (s, bidx, ids, step), want, _ = KI.order_expected(65, 16)
    sampler, s64 = SO.Sampler(KI.SEED), s.astype(np.float64)
    got = sampler.order(step, [int(v) for v in ids[bidx]], np.exp(s64), s64)
    assert np.array_equal(got, want) and sampler.n_masked_rows >= 16 and np.isfinite(sampler.order_margin)
    masked = s < -500
    assert (np.exp(s64)[masked] == 0).all()
    tails = [list(got[r, 16 - int(masked[r].sum()):]) for r in range(65) if masked[r].sum() >= 2]
    assert any(t != sorted(t) for t in tails)           # (index order would be another order)


def test_seed_none_follows_torch_manual_seed():
    g = SF.load(*CASES[0])
    be, d = DrawingOracle.of(g.kind), g.decoder()       # (building a module draws its initial weights)
    torch.manual_seed(77)
    lo, hi = G.split_seed(None)
    torch.manual_seed(77)
    (a, ma), _ = _sampled(g, None, backend=be, d=d)
    torch.manual_seed(77)
    (b, mb), _ = _sampled(g, None, backend=be, d=d)
    (c, mc), _ = _sampled(g, lo | hi << 32, backend=be, d=d)
    assert norm(a) == norm(b) == norm(c) and ma == mb == mc
    torch.manual_seed(78)
    assert G.split_seed(None) != (lo, hi)
    assert G.split_seed(0x123456789ABCDEF0) == (0x9ABCDEF0, 0x12345678) and G.split_seed(-1) == (0xFFFFFFFF, 0xFFFFFFFF)


def test_a_backend_without_draws_needs_a_sampler():
    g = SF.load(*CASES[0])
    with pytest.raises(TypeError, match="sampler"):
        SF.decode_sampled(g, g.decoder(), g.latents("cpu"), seed=1, backend=SF.oracle_backend(g.kind))


@pytest.mark.parametrize("kind", ["motif", "hier"])
def test_entry_points(kind):
    g = SF.load(*[c for c in CASES if c[0] == kind][0])
    d, gb, name = g.decoder(), SF.graph_batch(kind), {"motif": "MotifDecoder", "hier": "HierMPNDecoder"}[kind]
    z = (None, None, None)
    with pytest.raises(NotImplementedError, match="greedy") as e:       # decode(greedy=False) still refuses ...
        d.decode(None, z, greedy=False, graph_batch_factory=gb)
    assert name + ".decode_sampled" in str(e.value)                     # ... and says where sampling lives
    # decode_sampled makes decode's refusals: no graph batch, active dropout, the beam limits, one id per molecule
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        d.decode_sampled(None, z, seed=1)
    lat = g.latents("cpu")
    for beam in (0, 13, 17):
        with pytest.raises(ValueError, match="beam"):
            d.decode_sampled(None, lat, seed=1, beam=beam, graph_batch_factory=gb)
    with pytest.raises(ValueError, match="sample_ids"):
        d.decode_sampled(None, lat, seed=1, sample_ids=[0, 1], graph_batch_factory=gb)
    if kind == "motif":
        from motif_fixtures import MotifGolden
        wet = MotifGolden("prop_gru_s60").model(dropout=0.1).decoder.train()
    else:
        import hier_decode_fixtures as HF
        wet = HF.hier_decoder("GRU", 16, 8, 12, 36, 1, 1, 1, 0.0, dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="eval"):
        wet.decode_sampled(None, z, seed=1, graph_batch_factory=gb)


def test_sample_is_on_every_model_and_refuses_like_reconstruct():
    from ggpm_amd import property_vae as PV
    for cls in (PV.HierPropertyVAE, PV.HierPropOptVAE, PV.PropertyVAE, PV.PropOptVAE):
        assert callable(getattr(cls, "sample"))
    from motif_fixtures import MotifGolden
    m = MotifGolden("prop_gru_s60").model()
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        m.sample(2, seed=1)
    wet = MotifGolden("prop_gru_s60").model(dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="eval"):
        wet.sample(2, seed=1, graph_batch_factory=SF.graph_batch("motif"))
