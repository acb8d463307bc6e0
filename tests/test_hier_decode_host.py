"""CPU: the host side of HierMPNDecoder.decode -- SynthHierGraphBatch's atom tables and DecodeTree's tree tables with
cgraph against the reference's own (tests/golden/hier_decode), the changed-row detection, the whole host loop on the fp64
restatement of the kernels (tests/hier_decode_kernel_oracle.py) against the reference's recorded decode, and the entry
points' refusals."""
import numpy as np
import pytest
import torch

import hier_decode_fixtures as HF
import hier_decode_kernel_oracle as HO
from ggpm_amd import hier_decode as HD
from ggpm_amd.motif_decode import DecodeTree
from ggpm_amd.synth_graph import SynthAtomVocab, SynthHierGraphBatch
from ggpm_amd.vocab import IndexPairVocab


@pytest.mark.parametrize("name", HF.names())
def test_add_mol_replay_gives_the_reference_atom_tables(name):
    g = HF.HierDecodeGolden(name)
    gb = SynthHierGraphBatch(IndexPairVocab(g.n_motif, g.n_attach), SynthAtomVocab(), g.B, node_fdim=38, edge_fdim=62)
    for bid, ismiles, inter_label, nth, want in g.add_mol:
        got = gb.add_mol(bid, ismiles, [tuple(p) for p in inter_label], nth)
        assert [list(map(int, o)) for o in got] == want
    fnode, fmess, agraph, bgraph, _ = gb.get_tensors()
    assert fnode.shape == (100 * g.B, 38) and fmess.shape == (300 * g.B, 62)
    assert agraph.shape == bgraph.shape == (300 * g.B, 10)
    for t, (k, want) in zip((fnode, fmess, agraph, bgraph), g.atom_tables().items()):
        assert np.array_equal(t.numpy()[:len(want)], want), k
        assert not t.numpy()[len(want):].any(), k
    assert gb.get_mol() == g.mols


@pytest.mark.parametrize("name", HF.names())
def test_tree_replay_gives_the_reference_tree_tables(name):
    g = HF.HierDecodeGolden(name)
    tree = DecodeTree(100 * g.B, 200 * g.B, 12, cgraph=True)
    mirror = {k: np.zeros_like(v) for k, v in g.tree_tables().items()}
    for op in g.ops:
        if op[0] == "node":
            tree.add_node()
        elif op[0] == "edge":
            tree.add_edge(op[1], op[2], None if op[3] is None else tuple(op[3]))
        elif op[0] == "feat":
            tree.set_node_feature(op[1], op[2], op[3])
        else:
            tree.register_cgraph(op[1], op[2], op[3], op[4])
    for k, want in g.tree_tables().items():
        assert np.array_equal(getattr(tree, k)[:len(want)], want), k
    # the queued edits alone rebuild the tables (what the device copy receives)
    ne, te = tree.take_edits()
    for n, v in ne:
        mirror["fnode"][n, 0] = v
    for tab, row, slot, v in te:
        if tab == 2:
            mirror["fmess"][row, (0, 2)[slot]] = v
        else:
            mirror[{0: "agraph", 1: "bgraph", 3: "fnode", 4: "cgraph"}[tab]][row, slot] = v
    want = g.tree_tables()
    want["fmess"] = want["fmess"].copy()
    want["fmess"][:, 1] = 0            # (the destination node is not sent)
    for k in want:
        assert np.array_equal(mirror[k], want[k]), k


def test_decode_tree_defaults_are_the_tree_only_ones():
    tree = DecodeTree(8, 8)
    assert tree.cgraph is None and tree.agraph.shape == (8, 12)
    a, b = tree.add_node(), tree.add_node()
    tree.add_edge(a, b, (a, b, 0))
    tree.set_node_feature(b, 3, 4)
    tree.register_cgraph(b, [1, 2], [1, 2], [])
    ne, te = tree.take_edits()
    assert ne == [(b, 3)] and all(tab in (0, 1, 2) for tab, _, _, _ in te)


def test_changed_rows_finds_exactly_the_rows_that_differ():
    rs = np.random.RandomState(0)
    host = rs.standard_normal((40, 7)).astype(np.float32)
    shadow = host.copy()
    assert len(HD.changed_rows(host, shadow, 40)) == 0
    host[3, 6] += 1
    host[17] = 0
    host[39, 0] = 5            # beyond the used prefix
    assert HD.changed_rows(host, shadow, 39).tolist() == [3, 17]
    assert np.array_equal(shadow[:39], host[:39]) and shadow[39, 0] != 5
    assert HD.changed_rows(host, shadow, 40).tolist() == [39]
    assert HD.changed_rows(host, shadow, 0).tolist() == []


def test_atom_tables_edits_come_from_the_tables_alone():
    """a graph batch that never says what it touched: the rows found are those its add_mol wrote"""
    gb = SynthHierGraphBatch(IndexPairVocab(12, 36), SynthAtomVocab(), 2, node_fdim=38, edge_fdim=62)
    tabs = HD.AtomTables(gb.get_tensors())
    out = gb.add_mol(0, "a1", [], 0)             # a 5-ring: atoms 1..5, messages 1..10
    tabs.note(out[0], out[1])
    fn, fm, ag, bg = tabs.take_edits()
    assert len(fn[0]) == 0                       # add_node drops the feature: no fnode row changes
    assert fm[0].tolist() == list(range(1, 11)) and ag[0].tolist() == [1, 2, 3, 4, 5]
    assert bg[0].tolist() == list(range(1, 11)) and np.array_equal(bg[1], gb.bgraph.numpy()[1:11])
    assert all(len(r) == 0 for r, _ in tabs.take_edits())
    out = gb.add_mol(0, "a0", [(2, 0)], 1)       # a bond at atom 2
    tabs.note(out[0], out[1])
    fn, fm, ag, bg = tabs.take_edits()
    assert fm[0].tolist() == [11, 12] and ag[0].tolist() == [2, 6]
    # message 11 = (2 -> 6) reads the two ring messages into atom 2; message 12 = (6 -> 2) is read by the messages leaving
    # atom 2 along the ring, 2 = (2 -> 1) and 3 = (2 -> 3); its own row stays zero (atom 6 has no other neighbour)
    assert bg[0].tolist() == [2, 3, 11] and all(np.array_equal(v, gb.bgraph.numpy()[r]) for r, v in zip(*bg))


@pytest.mark.parametrize("name", HF.names())
def test_host_loop_on_the_fp64_kernels_reproduces_the_reference(name):
    g = HF.HierDecodeGolden(name)
    d = g.decoder()
    made = []

    def factory(*a, **k):
        made.append(SynthHierGraphBatch(*a, **k))
        return made[-1]
    results, mols = HD.decode(d, None, g.latents(), max_decode_step=g.max_step, beam=g.beam, graph_batch_factory=factory,
                              backend=HO.OracleBackend)
    g.check(d, results, mols, made[0])


def test_fixtures_cover_the_branches():
    seen = {k for n in HF.names() for k, v in HF.HierDecodeGolden(n).features.items() if v}
    assert seen >= {"several_candidates", "distinct_scores", "two_atom_attachments", "no_candidate", "refusals",
                    "forced_backtrack", "early_empty", "stopped_at_max"}
    gs = [HF.HierDecodeGolden(n) for n in HF.names()]
    assert {g.rnn for g in gs} == {"GRU", "LSTM"} and {g.diterG for g in gs} >= {1, 3} and {g.diterT for g in gs} >= {1, 2}
    assert any(g.L != g.H for g in gs) and all(float(g.z["margin"]) >= 1e-4 for g in gs)


class _Search:
    optimize_type, property_optim_step, patience, patience_threshold = "fixed", 5, 3, 0.01
    property_delta, latent_lr, max_steps = 0.01, 0.05, 10000


def test_entry_points_without_a_graph_batch_raise():
    import property_fixtures as pf
    from golden_utils import VaeGolden
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    from ggpm_amd.property_vae import HierPropertyVAE, HierPropOptVAE
    g = pf.PropOptGolden(pf.names("propopt")[0])
    m = HierPropOptVAE(g.args(IndexPairVocab(g.n_motif, g.n_attach)))
    v = VaeGolden("vae_gru_s42")
    p = HierPropertyVAE(v.args(IndexPairVocab(v.n_motif, v.n_attach)))
    for model in (p, m):
        with pytest.raises(NotImplementedError, match="graph_batch_factory"):
            model.reconstruct(None, None)
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        HierPropertyVAEOptimizer(m, _Search()).forward(None, _Search())
    with pytest.raises(NotImplementedError, match="graph_batch_factory"):
        p.decoder.decode(None, (None, None, None))
    with pytest.raises(NotImplementedError, match="greedy"):
        p.decoder.decode(None, (None, None, None), greedy=False, graph_batch_factory=SynthHierGraphBatch)
    d = HF.hier_decoder("GRU", 16, 8, 12, 36, 1, 1, 1, 0.0, dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="eval"):
        d.decode(None, (None, None, None), graph_batch_factory=SynthHierGraphBatch)


def test_shapes_outside_the_limits_raise_before_any_launch():
    d = HF.hier_decoder("GRU", 16, 8, 12, 36, 1, 1, 1, 0.0)
    z = tuple(torch.zeros(2, 8) for _ in range(3))
    with pytest.raises(ValueError, match="beam"):
        d.decode(None, z, beam=17, graph_batch_factory=SynthHierGraphBatch)
    with pytest.raises(ValueError, match="beam"):
        d.decode(None, z, beam=0, graph_batch_factory=SynthHierGraphBatch)

    class Wide(SynthHierGraphBatch):
        def __init__(self, *a, **k):
            super().__init__(*a, **dict(k, max_nb=12))
    with pytest.raises(ValueError, match="atom tables"):
        d.decode(None, z, graph_batch_factory=Wide)


def test_what_the_graph_batch_raises_is_raised():
    """the reference's hierarchical decode has no try/except: an exception of an entry the assembly reaches ends the
    decode; one of an entry it never reaches does not"""
    g = HF.HierDecodeGolden("gru_h16_g3")
    d = g.decoder()

    class Boom(SynthHierGraphBatch):
        calls = 0

        def get_assm_cands(self, *a):
            Boom.calls += 1
            if Boom.calls == 1:
                raise KeyError("no such fragment")
            return super().get_assm_cands(*a)
    with pytest.raises(KeyError, match="no such fragment"):
        HD.decode(d, None, g.latents(), max_decode_step=g.max_step, beam=g.beam, graph_batch_factory=Boom,
                  backend=HO.OracleBackend)
