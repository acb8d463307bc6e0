"""GPU: HierMPNDecoder.decode on the HIP kernels against the reference's own decode (tests/golden/hier_decode); the
reconstruct forms and HierPropertyVAEOptimizer.forward; run-to-run and batch-composition invariance; the device mirrors of
every table after edits on both sides of the 64-lane and 256-thread boundaries; the per-step launch, upload and copy
counts."""
import numpy as np
import pytest
import torch

import hier_decode_fixtures as HF
from decode_fixtures import assert_same, norm
from ggpm_amd import hier_decode as HD
from ggpm_amd.synth_graph import SynthAtomVocab, SynthHierGraphBatch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _decode(d, z, steps, beam=5, factory=SynthHierGraphBatch):
    return d.decode(None, z, max_decode_step=steps, beam=beam, graph_batch_factory=factory)


def _roomy(*a, **k):
    """atom tables that hold a molecule of 20 expansions when it is alone in its batch (IncGraph's 100 atoms and 300
    messages per molecule are shared by the batch; a molecule alone has no neighbour's share to grow into)"""
    return SynthHierGraphBatch(*a, max_nodes=400, max_edges=1200, **k)


@pytest.mark.parametrize("name", HF.names())
def test_decode_matches_the_reference(name):
    g = HF.HierDecodeGolden(name)
    d = g.decoder(DEV)
    made = []

    def factory(*a, **k):
        made.append(SynthHierGraphBatch(*a, **k))
        return made[-1]
    results, mols = d.decode(None, g.latents(DEV), max_decode_step=g.max_step, beam=g.beam, graph_batch_factory=factory)
    g.check(d, results, mols, made[0])


def test_two_runs_are_bit_identical():
    g = HF.HierDecodeGolden("lstm_h16_g3")
    d = g.decoder(DEV)
    a = norm(_decode(d, g.latents(DEV), g.max_step))
    b = norm(_decode(d, g.latents(DEV), g.max_step))
    assert a == b


def _latents(B, L, seed):
    rs = np.random.RandomState(seed)
    return tuple(torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).to(DEV) for _ in range(3))


def _decisions(entries):
    """one molecule's results without the graph batch's global atom ids"""
    out = []
    for e in norm(entries):
        e = dict(e)
        af = e.get("Attaching Fragment")
        if isinstance(af, dict):
            e["Attaching Fragment"] = {k: v for k, v in af.items() if k != "attachment-points"}
        elif af is not None:
            e["Attaching Fragment"] = [af[0], af[1], af[3]]
        out.append(e)
    return out


@pytest.mark.parametrize("rnn,H,L,B", [("LSTM", 250, 24, 8), ("GRU", 300, 32, 8)])
def test_batch_composition_invariance(rnn, H, L, B):
    """each molecule decoded alone makes the decisions it makes within the batch (every kernel computes a row from that
    row's inputs alone, in a fixed order)"""
    d = HF.hier_decoder(rnn, H, L, 50, 150, 1, 3, 11, 0.5).to(DEV)
    z = _latents(B, L, 12)
    results, mols = _decode(d, z, 20, factory=_roomy)
    for b in range(B):
        r1, m1 = _decode(d, tuple(v[b:b + 1] for v in z), 20, factory=_roomy)
        alone = _decisions(r1[0])
        if alone[-1] == {}:             # the loop ended when this molecule's stack emptied
            alone = alone[:-1]
        within = _decisions(results[b])
        assert_same(alone, within[:len(alone)], tol=1e-5, path="molecule %d" % b)
        assert all(set(e) == {"partial-graph"} for e in within[len(alone):])
        assert m1[0] == mols[b]


def test_device_mirrors_equal_the_host_tables():
    """70 molecules, a bias that makes every molecule expand at every step, 6 steps: tree and atom edits on both sides of
    the 64-lane and 256-thread boundaries of the edit kernel.  The device tables, read back once after the loop, against
    the host's (the last step's assembly edits are not uploaded -- no step reads them -- and are applied here)."""
    d = HF.hier_decoder("GRU", 32, 16, 24, 72, 1, 1, 21, 3.0).to(DEV)
    z = _latents(70, 16, 22)
    run = HD._Decode(d, SynthHierGraphBatch, z, 6, 8)
    with torch.no_grad():
        run.run()
    got = run.be.tables()
    tree, n, e = run.tree, run.tree.n_nodes, run.tree.n_edges
    assert n > 256
    for tab, row, slot, v in run._tree_edits():
        got[{0: "t_agraph", 1: "t_bgraph", 2: "t_fmess", 3: "t_fnode", 4: "t_cgraph"}[int(tab)]][row, slot] = v
    for name, (rows, vals) in zip(("a_fnode", "a_fmess", "a_agraph", "a_bgraph"), run.atab.take_edits()):
        got[name][rows] = vals
    assert np.array_equal(got["t_fnode"][:n], tree.fnode[:n])
    assert np.array_equal(got["t_fmess"][:e], tree.fmess[:e][:, (0, 2)])
    assert np.array_equal(got["t_agraph"][:n], tree.agraph[:n]) and np.array_equal(got["t_bgraph"][:e], tree.bgraph[:e])
    assert np.array_equal(got["t_cgraph"][:n], tree.cgraph[:n]) and tree.cgraph[:n].any()
    fn, fm, ag, bg = run.atab.host
    na, ea = run.atab.n_atoms, run.atab.n_mess
    assert na > 256 and ea > 256
    assert np.array_equal(got["a_fnode"][:na], fn[:na]) and np.array_equal(got["a_fmess"][:ea], fm[:ea])
    assert np.array_equal(got["a_agraph"][:na], ag[:na]) and np.array_equal(got["a_bgraph"][:ea], bg[:ea])
    for k, t in got.items():            # nothing was written past the used prefixes
        used = {"t_fnode": n, "t_agraph": n, "t_cgraph": n, "t_fmess": e, "t_bgraph": e, "a_fnode": na,
                "a_agraph": na}.get(k, ea)
        assert not t[used:].any(), k


@pytest.mark.parametrize("name", HF.names())
def test_per_step_launch_upload_and_copy_counts(name):
    """the constants of DESIGN (hier_decode.LAUNCHES): a step's phases each cost a fixed number of launches, one upload
    and one copy back, whatever the batch, the clusters and the candidates"""
    g = HF.HierDecodeGolden(name)
    d = g.decoder(DEV)
    _decode(d, g.latents(DEV), g.max_step, g.beam)
    topo, expand, score = HD.LAUNCHES(g.diterG, g.diterT)
    assert (topo, expand, score) == (5 + g.diterG, 10, 1)
    kinds = set()
    for s in d.last_decode_stats:
        n = 1 + s["expand"] + s["scored"] if s["mess"] else 1
        assert s["scored"] <= s["expand"] <= s["mess"]
        want = topo + (5 if s["mess"] else 0) + (expand - 5) * s["expand"] + score * s["scored"]
        assert (s["launches"], s["h2d"], s["d2h"]) == (want, 1 + s["mess"] + s["scored"], n), s
        assert s["launches"] <= topo + expand + score and s["h2d"] <= 3 and s["d2h"] <= 3
        kinds.add((s["mess"], s["expand"], s["scored"]))
    assert (1, 1, 1) in kinds         # every fixture has steps that run all three phases


class _Args:
    graph_batch_factory = SynthHierGraphBatch
    optimize_type, property_optim_step, patience, patience_threshold = "fixed", 5, 3, 0.01
    property_delta, latent_lr, max_steps = 0.01, 0.05, 10000


def _hier(kind, name):
    import property_fixtures as pf
    from golden_utils import VaeGolden
    from ggpm_amd import synth
    from ggpm_amd.property_vae import HierPropertyVAE, HierPropOptVAE
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name) if kind == "hier-prop" else pf.PropOptGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.atom_vocab = SynthAtomVocab()
    model = (HierPropertyVAE if kind == "hier-prop" else HierPropOptVAE)(args).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=False)
    tensors = synth.tensorize(g.specs())
    homos, lumos = (None, None) if kind == "hier-prop" else (g.z["t_homo"].tolist(), g.z["t_lumo"].tolist())
    return model.eval(), (None, None, tensors, [None] * g.B, homos, lumos)


def test_reconstruct_hier_prop():
    from ggpm_amd.nnutils import make_cuda
    from ggpm_amd.property_vae import rsample
    m, batch = _hier("hier-prop", "vae_gru_s42")
    got = m.reconstruct(batch, _Args())
    with torch.no_grad():
        tree_tensors, graph_tensors = make_cuda(batch[2])
        z, _ = rsample(m.encoder.forward_padded(tree_tensors, graph_tensors)[0], m.R_mean, m.R_var, perturb=False)
    want = _decode(m.decoder, (z, z, z), 150)
    assert norm(got) == norm(want)
    assert len(got[0][0]) > 2
    m.decoder.graph_batch_factory = SynthHierGraphBatch       # the decoder's factory when args names none
    assert norm(m.reconstruct(batch, None)) == norm(want)


def test_reconstruct_hier_prop_opt_and_optimizer_forward():
    import property_fixtures as pf
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    m, batch = _hier("hier-prop-opt", pf.names("propopt")[0])
    props, rec = m.reconstruct(batch, _Args())
    for a, b in zip(props, m.predict_properties(batch)):
        assert torch.equal(a, b)
    with torch.no_grad():
        z, _ = m.encode_latent(batch[2], perturb=False)
    assert norm(rec) == norm(_decode(m.decoder, (z, z, z), 150))
    opt = HierPropertyVAEOptimizer(m, _Args())
    props2, rec2 = opt.forward(batch, _Args())
    latent, _ = opt.optimize(batch)
    assert norm(rec2) == norm(_decode(m.decoder, (latent, latent, latent), 150))
    half = m.latent_size
    for a, b in zip(props2, m.property_optim.predict(homo_vecs=latent[:, :half], lumo_vecs=latent[:, half:])):
        assert torch.equal(a, b)
