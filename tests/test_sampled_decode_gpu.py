"""GPU: ``decode_sampled`` of both decoders on the HIP backend -- the device draws against the fp64 oracle backend with the
restated sampler at the same seed, the reference's recorded sampled decodes replayed through the ``sampler=`` seam, the
per-step launch, upload and copy counts against the greedy step's, the invariance of a molecule's decode to its batch --
and ``sample`` of the four VAEs."""
import numpy as np
import pytest
import torch

import sample_oracle as SO
import sampled_decode_fixtures as SF
from decode_fixtures import assert_same, norm

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
CASES = SF.cases()
IDS = [kind + "-" + name for kind, name in CASES]
SAMPLE_IDS = [10, 11, 12, 13]


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_device_draws_equal_the_oracle_with_the_restated_sampler(kind, name):
    g = SF.load(kind, name)
    sampler = SO.Sampler(SF.SEED)
    want = SF.decode_sampled(g, g.decoder(), g.latents("cpu"), seed=SF.SEED, sample_ids=SAMPLE_IDS,
                             backend=SF.oracle_backend(kind), sampler=sampler)
    # the fp32 heads can be asked to decide as fp64 does only where the draw is not on the edge
    print("margins: topology %.3e, keys %.3e" % (sampler.topo_margin, sampler.order_margin))
    assert sampler.topo_margin >= SO.MARGIN and sampler.order_margin >= SO.MARGIN
    d = g.decoder(DEV)
    got = SF.decode_sampled(g, d, g.latents(DEV), seed=SF.SEED, sample_ids=SAMPLE_IDS)
    assert_same(norm(got[0]), norm(want[0]))
    assert norm(got[1]) == norm(want[1])
    again = SF.decode_sampled(g, d, g.latents(DEV), seed=SF.SEED, sample_ids=SAMPLE_IDS)
    assert norm(again) == norm(got)                                 # the same seed: bit for bit
    # molecules 1 and 3 alone, under their own ids
    rs, ms = SF.decode_sampled(g, d, g.latents(DEV), rows=[1, 3], seed=SF.SEED, sample_ids=[11, 13])
    for j, b in enumerate((1, 3)):
        assert_same(SF.own(rs[j]), SF.own(got[0][b]), tol=1e-5, path="molecule %d" % b)
        assert ms[j] == got[1][b]


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_replaying_the_reference_draws_on_the_device(kind, name):
    g = SF.load(kind, name)
    d, replay = g.decoder(DEV), g.replay()
    made = []

    def factory(*a, **k):
        made.append(SF.graph_batch(kind)(*a, **k))
        return made[-1]
    results, mols = SF.module(kind).decode_sampled(d, None, g.latents(DEV), max_decode_step=g.max_step, beam=g.beam,
                                                   graph_batch_factory=factory, sampler=replay)
    assert replay.exhausted()
    if kind == "hier":
        g.check(d, results, mols, made[0])
    else:
        g.check(d, results, mols)


def _greedy_cost(g, s):
    """(launches, uploads, copies back) of a greedy step with the phases of ``s``: the constants of the two backends"""
    from ggpm_amd import greedy_decode as G
    from ggpm_amd import hier_decode as HD
    from ggpm_amd import motif_decode as MD
    if g.kind == "motif":
        launches = (MD.L_TREE + G.L_MLP) + MD.L_TREE + s["expand"] * (2 * G.L_MLP + G.L_TOPK) + s["scored"] * G.L_ASSM
        return launches, 2 + s["scored"], 1 + s["expand"] + s["scored"]
    topo, expand, score = HD.LAUNCHES(g.diterG, g.diterT)
    launches = topo + (5 if s["mess"] else 0) + (expand - 5) * s["expand"] + score * s["scored"]
    return launches, 1 + s["mess"] + s["scored"], 1 + s["expand"] + s["scored"]


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_a_sampled_step_costs_the_greedy_step_and_at_most_two_launches(kind, name):
    g = SF.load(kind, name)
    d = g.decoder(DEV)
    SF.module(kind).decode(d, None, g.latents(DEV), max_decode_step=g.max_step, beam=g.beam,
                           graph_batch_factory=SF.graph_batch(kind))
    for s in d.last_decode_stats:               # what a greedy step costs, phase by phase
        assert (s["launches"], s["h2d"], s["d2h"]) == _greedy_cost(g, s), s
    SF.decode_sampled(g, d, g.latents(DEV), seed=SF.SEED)
    seen = set()
    for s in d.last_decode_stats:
        launches, h2d, d2h = _greedy_cost(g, s)
        assert (s["h2d"], s["d2h"]) == (h2d, d2h), s
        assert s["launches"] == launches + 1 + s["expand"] <= launches + 2, s     # the topology draw, the order draw
        seen.add((s["mess"], s["expand"], s["scored"]))
    assert (1, 1, 1) in seen and len(seen) >= 2
    # with a host sampler no draw kernel runs: the greedy step's launches
    SF.decode_sampled(g, d, g.latents(DEV), seed=SF.SEED, sampler=SO.Sampler(SF.SEED))
    for s in d.last_decode_stats:
        assert (s["launches"], s["h2d"], s["d2h"]) == _greedy_cost(g, s), s


def _motif(name):
    from motif_fixtures import MotifGolden
    return MotifGolden(name).model().to(DEV).eval()


def _hier(which, name):
    import property_fixtures as pf
    from golden_utils import VaeGolden
    from ggpm_amd.property_vae import HierPropertyVAE, HierPropOptVAE
    from ggpm_amd.synth_graph import SynthAtomVocab
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name) if which == "prop" else pf.PropOptGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.atom_vocab = SynthAtomVocab()
    model = (HierPropertyVAE if which == "prop" else HierPropOptVAE)(args).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=False)
    return model.eval()


def _models():
    import property_fixtures as pf
    return [("PropertyVAE", "motif", lambda: _motif("prop_lstm_s61")),
            ("PropOptVAE", "motif", lambda: _motif("propopt_gru_s63")),
            ("HierPropertyVAE", "hier", lambda: _hier("prop", "vae_gru_s42")),
            ("HierPropOptVAE", "hier", lambda: _hier("propopt", pf.names("propopt")[0]))]


@pytest.mark.parametrize("name,kind,make", _models(), ids=[m[0] for m in _models()])
def test_sample(name, kind, make):
    m = make()
    assert type(m).__name__ == name
    gb, seed, steps = SF.graph_batch(kind), 0xABCDEF0123456789, 12
    results, mols = m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb)
    from ggpm_amd import functional as F_
    width = m.decoder.latent_size           # what reconstruct hands to decode
    z = F_.sample_normal(4, width, *SO.split(seed), device=DEV)
    assert len(results) == len(mols) == 4 and all(isinstance(s, str) and s for s in mols)
    # the latents: the restated normals of ids 0..3
    ids = np.arange(4)
    want = SO.normals(seed, ids, width)
    bound = 4.0 * float(np.abs(SO.normals(seed, ids, width, np.float32).astype(np.float64) - want).max())
    assert z.shape == (4, width) and float(np.abs(z.cpu().numpy().astype(np.float64) - want).max()) <= bound
    # greedy=True continues into decode on those latents
    assert norm((results, mols)) == norm(m.decoder.decode(None, (z, z, z), max_decode_step=steps, graph_batch_factory=gb))
    assert norm(m.sample(4, seed=seed, max_decode_step=steps, graph_batch_factory=gb)) == norm((results, mols))
    # greedy=False: the same latents, then decode_sampled at the same seed; the decoder's own factory when none is named
    m.decoder.graph_batch_factory = gb
    a = m.sample(4, greedy=False, seed=seed, max_decode_step=steps)
    assert norm(a) == norm(m.decoder.decode_sampled(None, (z, z, z), seed=seed, max_decode_step=steps))
    assert norm(a) == norm(m.sample(4, greedy=False, seed=seed, max_decode_step=steps))
    torch.manual_seed(3)
    b = m.sample(4, greedy=False, max_decode_step=steps)
    torch.manual_seed(3)
    assert norm(b) == norm(m.sample(4, greedy=False, max_decode_step=steps))
    draws = {e["Generate fragment"] for r in norm(a[0]) for e in r[1:] if "Generate fragment" in e}
    assert draws <= {0.0, 1.0} and draws
