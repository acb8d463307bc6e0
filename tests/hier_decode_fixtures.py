"""The hierarchical decode fixtures (tests/golden/make_golden_hier_decode.py): loading, the decoder they were made with,
and the comparison of a decode against the reference's."""
import glob
import json
import os

import numpy as np
import torch

from decode_fixtures import assert_same, norm, state_dict

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hier_decode")
TREE_TABLES = ("fnode", "fmess", "agraph", "bgraph", "cgraph")
ATOM_TABLES = ("fnode", "fmess", "agraph", "bgraph")


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def hier_decoder(rnn, H, L, n_motif, n_attach, diterT, diterG, seed, topo_bias, param_names=None, dropout=0.0):
    """a HierMPNDecoder (CPU, eval) with seeded_state_dict weights over ``param_names`` (default: its own order)"""
    from ggpm_amd.decoder import HierMPNDecoder
    from ggpm_amd.synth_graph import SynthAtomVocab
    from ggpm_amd.vocab import IndexPairVocab
    d = HierMPNDecoder(IndexPairVocab(n_motif, n_attach), SynthAtomVocab(), rnn, H, H, L, diterT, diterG, dropout)
    if param_names is None:
        param_names = [k for k, _ in d.named_parameters()]
    d.load_state_dict(state_dict(d, param_names, seed, topo_bias), strict=True)
    return d.eval()


class HierDecodeGolden:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        (self.H, self.L, self.diterT, self.diterG, self.B, self.n_motif, self.n_attach, self.max_step, self.beam,
         self.seed) = [int(v) for v in self.z["meta"]]
        self.rnn, self.topo_bias = str(self.z["rnn"]), float(self.z["topo_bias"])
        for k in ("results", "mols", "cands", "ops", "add_mol", "features"):
            setattr(self, k, json.loads(str(self.z[k])))

    def decoder(self, device=None):
        d = hier_decoder(self.rnn, self.H, self.L, self.n_motif, self.n_attach, self.diterT, self.diterG, self.seed,
                         self.topo_bias, [str(k) for k in self.z["param_names"]])
        return d if device is None else d.to(device)

    def latents(self, device="cpu"):
        return tuple(torch.from_numpy(self.z[k]).to(device) for k in ("root_vecs", "tree_vecs", "graph_vecs"))

    def tree_tables(self):
        return {k: self.z["tree_" + k] for k in TREE_TABLES}

    def atom_tables(self):
        return {k: self.z["atom_" + k] for k in ATOM_TABLES}

    def check(self, dec, results, mols, graph_batch=None):
        """a decode's results, molecules, tried candidates with their scores and final tables against the reference's"""
        assert_same(norm(results), self.results)
        assert norm(mols) == self.mols
        trace = [[c, s] for (_, _, _, c, s) in dec.last_decode_trace]
        assert [c for c, _ in trace] == [c for c, _ in self.cands]
        for (_, s), (_, w) in zip(trace, self.cands):
            assert_same(s, w, path="attachment scores")
        tree = dec.last_decode_tree
        tabs = self.tree_tables()
        assert tree.n_nodes == len(tabs["fnode"]) and tree.n_edges == len(tabs["fmess"])
        for k, want in tabs.items():
            assert np.array_equal(getattr(tree, k)[:len(want)], want), k
        if graph_batch is not None:
            for t, (k, want) in zip(graph_batch.get_tensors(), self.atom_tables().items()):
                assert np.array_equal(t.numpy()[:len(want)], want), k
