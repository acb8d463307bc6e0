"""CPU: the synthetic graph batch, the vocabulary's label strings, the decode's host bookkeeping against the reference's
tables, the whole host loop on the fp64 restatement of the kernels (tests/decode_kernel_oracle.py) against the reference's
recorded decode, the two decoders' error policies on one provocation, and the entry points that need a graph batch."""
import numpy as np
import pytest
import torch

import decode_kernel_oracle as O
from decode_fixtures import DecodeGolden, names
from ggpm_amd import motif_decode as MD
from ggpm_amd.motif_decode import DecodeTree
from ggpm_amd.synth_graph import SynthGraphBatch, fragment
from ggpm_amd.vocab import IndexPairVocab


def test_fragment_rules():
    assert fragment("a0") == (2, ["C", "N"], 1)
    assert fragment("a1")[0] == 5 and fragment("a2")[0] == 6
    assert fragment("a7") == (5, ["O", "S", "C", "N", "O"], 2)      # a 5-ring with j % 4 == 3 shares a bond
    assert fragment("a3")[2] == 1                                   # a bond never does


def _ring_batch():
    gb = SynthGraphBatch(IndexPairVocab(4, 12), None, 2, max_nodes=400, max_edges=500, node_fdim=38, edge_fdim=62)
    atoms, bonds, attached = gb.add_mol(0, "a2", [], 0)            # 6-ring C N O S C N
    return gb, atoms, bonds, attached


def test_synthetic_batch_branches():
    gb, atoms, bonds, attached = _ring_batch()
    assert len(atoms) == 6 and len(bonds) == 6 and attached == []
    cands, anchors, pts = gb.get_assm_cands(atoms, [], "a5")       # several candidates on a ring parent
    assert cands == [(a,) for a in atoms] and anchors == ["a5"] and pts == [0]
    # a ring child adds 2 bonds at C (2 + 2 <= 4), not at N (> 3) or O (> 2); a bond child adds 1 at N, not at O
    assert gb.try_add_mol(0, "a5", [(atoms[0], 0)]) and not gb.try_add_mol(0, "a5", [(atoms[1], 0)])
    assert not gb.try_add_mol(0, "a5", [(atoms[2], 0)])
    assert gb.try_add_mol(0, "a3", [(atoms[1], 0)]) and not gb.try_add_mol(0, "a3", [(atoms[2], 0)])
    new, _, att = gb.add_mol(0, "a5", [(atoms[0], 0)], 1)
    assert new[0] == atoms[0] and att == [atoms[0]] and gb.degree[atoms[0]] == 4
    assert gb.get_assm_cands(atoms, list(atoms), "a5")[0] == []     # an exhausted parent: no candidate
    pairs = gb.get_assm_cands(atoms, [atoms[0]], "a7")[0]          # a fused ring: bonded pairs of unused atoms
    assert pairs == [(atoms[i], atoms[i + 1]) for i in range(1, 5)]
    assert gb.get_mol() == ["CNOSCNOSCNO|0-1,0-5,0-6,0-10,1-2,2-3,3-4,4-5,6-7,7-8,8-9,9-10"]


def test_synthetic_batch_is_deterministic():
    def run():
        gb, atoms, _, _ = _ring_batch()
        gb.add_mol(1, "a4", [], 0)
        gb.add_mol(0, "a7", [(atoms[1], 0), (atoms[2], 1)], 2)
        return gb.get_mol(), gb.degree, sorted(gb.bonds.items())
    assert run() == run()


def test_vocab_label_round_trip():
    v = IndexPairVocab(7, 21)
    for i in range(7):
        for j in (0, 5, 20):
            assert v[(v.get_smiles(i), v.get_ismiles(j))] == (i, j)
    assert v.get_smiles(torch.tensor(3)) == "m3" and v.get_ismiles(np.int64(4)) == "a4"


def test_fixtures_cover_the_branches():
    cases = [DecodeGolden(n) for n in names()]
    assert len(cases) >= 5 and {g.rnn for g in cases} == {"GRU", "LSTM"}
    assert {g.diterT for g in cases} == {1, 2} and {g.H == g.L for g in cases} == {True, False}
    for key in ("several_candidates", "no_candidate", "refusals", "forced_backtrack", "early_empty", "stopped_at_max",
                "two_atom_attachments"):
        assert any(g.features[key] for g in cases), key
    assert all(float(g.z["margin"]) >= 1e-4 for g in cases)


@pytest.mark.parametrize("name", names())
def test_tree_tables_match_the_reference(name):
    """DecodeTree replaying the reference's tree operations writes the reference's tables slot for slot, and hands the
    device one edit per node and per slot holding the last value."""
    g = DecodeGolden(name)
    tabs = g.tables()
    tree = DecodeTree(len(tabs["fnode"]) + 1, len(tabs["fmess"]) + 1)
    dev = {"fnode": np.zeros(tree.fnode.shape[0], np.int64), "fmess": np.zeros((tree.fmess.shape[0], 2), np.int64),
           "agraph": np.zeros_like(tree.agraph), "bgraph": np.zeros_like(tree.bgraph)}

    def apply():
        ne, te = tree.take_edits()
        assert len({n for n, _ in ne}) == len(ne) and len({e[:3] for e in te}) == len(te)
        for n, v in ne:
            dev["fnode"][n] = v
        for tab, row, slot, v in te:
            dev[("agraph", "bgraph", "fmess")[tab]][row, slot] = v
    for i, op in enumerate(g.ops):
        if op[0] == "node":
            tree.add_node()
        elif op[0] == "edge":
            tree.add_edge(op[1], op[2], op[3])
        else:
            tree.set_node_feature(op[1], op[2], op[3])
        if i % 7 == 6:
            apply()
    apply()
    assert tree.n_nodes == len(tabs["fnode"]) and tree.n_edges == len(tabs["fmess"])
    for k, want in tabs.items():
        assert np.array_equal(getattr(tree, k)[:len(want)], want), k
    assert np.array_equal(dev["fnode"][:len(tabs["fnode"])], tabs["fnode"][:, 0])
    assert np.array_equal(dev["fmess"][:len(tabs["fmess"])], tabs["fmess"][:, [0, 2]])
    for k in ("agraph", "bgraph"):
        assert np.array_equal(dev[k][:len(tabs[k])], tabs[k]), k


class _Search:
    optimize_type, property_optim_step, patience, patience_threshold = "fixed", 5, 3, 0.01
    property_delta, latent_lr, max_steps = 0.01, 0.05, 10000


def test_decode_entry_points_without_a_graph_batch_raise():
    from motif_fixtures import MotifGolden
    from ggpm_amd.property_control import PropertyVAEOptimizer
    p, m = MotifGolden("prop_gru_s60").model(), MotifGolden("propopt_gru_s63").model()
    for model in (p, m):
        with pytest.raises(NotImplementedError, match="graph_batch_factory"):
            model.reconstruct(None, None)
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        PropertyVAEOptimizer(m, _Search()).forward(None, _Search())
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        p.decoder.decode(None, (None, None, None))
    with pytest.raises(NotImplementedError, match="greedy"):
        p.decoder.decode(None, (None, None, None), greedy=False, graph_batch_factory=SynthGraphBatch)
    d = MotifGolden("prop_gru_s60").model(dropout=0.1).decoder.train()
    with pytest.raises(NotImplementedError, match="eval"):
        d.decode(None, (None, None, None), graph_batch_factory=SynthGraphBatch)


def _oracle_decode(g, factory=SynthGraphBatch):
    d = g.decoder()
    out = MD.decode(d, None, g.latents("cpu"), max_decode_step=g.max_step, beam=g.beam, graph_batch_factory=factory,
                    backend=O.OracleBackend)
    return d, out


@pytest.mark.parametrize("name", names())
def test_host_loop_on_the_fp64_kernels_reproduces_the_reference(name):
    g = DecodeGolden(name)
    d, (results, mols) = _oracle_decode(g)
    g.check(d, results, mols)
    for s, r in zip(d.last_decode_stats, zip(*[m[1:] for m in results])):
        # mess: a new message, that is a live molecule ('Generate fragment') that expanded or popped a node above its root
        assert s["scored"] <= s["expand"] <= s["mess"] <= 1
        assert s["expand"] == int(any("top-5-inter-cands" in e for e in r))


def _failing(method, exc):
    """a graph batch whose first call of ``method`` raises"""
    class Boom(SynthGraphBatch):
        calls = 0

    def first(self, *a):
        Boom.calls += 1
        if Boom.calls == 1:
            raise exc
        return getattr(SynthGraphBatch, method)(self, *a)
    setattr(Boom, method, first)
    return Boom


def _check_failed_expansion(g, d, results, t, bid, kk):
    """molecule ``bid``'s expansion of step ``t`` -- its first, so from its root -- failed at beam entry ``kk``: the entry
    lists the beam and attaches nothing; the new node keeps the feature of the entry that failed; the forced backtrack
    added the message back to the root, popped the root too (the stack is then empty: no third message), and the
    molecule's decode ended."""
    tree, vocab = d.last_decode_tree, d.vocab
    entry = results[bid][t + 1]
    assert "top-5-inter-cands" in entry and "Attaching Fragment" not in entry
    root = 2 + bid                              # node 0 the pad, 1 the super root, then one root per molecule
    assert len(tree.succs[root]) == 1
    new = tree.succs[root][0]
    assert tree.preds[root] == [1, new] and tree.preds[new] == [root] and tree.succs[new] == [root]
    assert tree.edge[(new, root)] > tree.edge[(root, new)]          # two messages: the expansion and the backtrack
    assert tuple(tree.fnode[new]) == tuple(vocab[entry["top-5-inter-cands"][kk][:2]])
    assert all(set(e) <= {"partial-graph"} for e in results[bid][t + 2:])
    assert len(results) == g.B and len(d.last_decode_stats) > t + 1


def test_tree_only_decode_catches_what_get_assm_cands_raises():
    """the provocation of test_hier_decode_host.test_what_the_graph_batch_raises_is_raised on the decoder whose reference
    has the try/except (decoder.py:1037): the entry that raised is the failed expansion, the decode goes on"""
    g = DecodeGolden("gru_h16")
    _, (clean, _) = _oracle_decode(g)
    # the first get_assm_cands: the first step in which a molecule expands, its first molecule, beam entry 0
    t, bid = min((t, b) for b, r in enumerate(clean) for t, e in enumerate(r[1:]) if "top-5-inter-cands" in e)
    boom = _failing("get_assm_cands", KeyError("no such fragment"))
    d, (results, mols) = _oracle_decode(g, boom)
    assert boom.calls > 1 and len(mols) == g.B
    _check_failed_expansion(g, d, results, t, bid, 0)


def test_tree_only_decode_catches_what_try_add_mol_raises():
    g = DecodeGolden("gru_h16")
    d0, _ = _oracle_decode(g)
    # the first try_add_mol: the first beam entry tried that has a candidate
    t, bid, kk = next((t, b, kk) for t, b, kk, cands, _ in d0.last_decode_trace if cands)
    boom = _failing("try_add_mol", RuntimeError("cannot attach"))
    d, (results, mols) = _oracle_decode(g, boom)
    assert boom.calls > 1 and len(mols) == g.B
    _check_failed_expansion(g, d, results, t, bid, kk)


def test_both_decoders_refuse_a_beam_outside_the_limits_alike():
    """1 to 16 and at most the vocabulary sizes (12 motifs here), before the graph batch or a backend is built"""
    import hier_decode_fixtures as HF
    from ggpm_amd import hier_decode as HD
    from ggpm_amd.synth_graph import SynthHierGraphBatch

    def never(*a, **k):
        raise AssertionError("built before the refusal")
    z = tuple(torch.zeros(2, 8) for _ in range(3))
    tree_only, hier = O.decoder("GRU", 16, 8, 12, 36), HF.hier_decoder("GRU", 16, 8, 12, 36, 1, 1, 1, 0.0)
    for beam in (0, 13, 17):
        said = []
        for mod, d, name in ((MD, tree_only, "MotifDecoder"), (HD, hier, "HierMPNDecoder")):
            with pytest.raises(ValueError, match="beam") as e:
                mod.decode(d, None, z, beam=beam, graph_batch_factory=never, backend=never)
            assert str(e.value).startswith(name + ".decode: ")
            said.append(str(e.value)[len(name):])
        assert said[0] == said[1] and "beam %d " % beam in said[0]
    for mod, d, factory in ((MD, tree_only, SynthGraphBatch), (HD, hier, SynthHierGraphBatch)):
        with pytest.raises(AssertionError, match="built before"):
            mod.decode(d, None, z, beam=12, graph_batch_factory=factory, backend=never)
