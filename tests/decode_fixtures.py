"""The decode fixtures (tests/golden/make_golden_decode.py): loading, the decoder they were made with, and the comparison
of a decode against the reference's."""
import glob
import json
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motif_decode")
TOL = 1e-4


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def canonical(key):
    """state_dict alias -> the parameter's own name (the decoder registers rnn_cell and E_assm twice)"""
    for alias, name in (("rnn_cell.", "hmpn.tree_encoder.rnn."), ("E_assm.", "hmpn.E_i.")):
        if key.startswith(alias):
            return name + key[len(alias):]
    return key


class AtomVocab:
    def size(self):
        return 38


def state_dict(model, param_names, seed, topo_bias):
    """seeded_state_dict over ``param_names`` (the reference's parameter order), topoNN's output bias raised by topo_bias"""
    from ggpm_amd.params import seeded_state_dict
    shapes = {canonical(k): tuple(v.shape) for k, v in model.state_dict().items()}
    sd = seeded_state_dict(OrderedDict((k, shapes[k]) for k in param_names), seed)
    sd["topoNN.3.bias"] = sd["topoNN.3.bias"] + np.float32(topo_bias)
    return OrderedDict((k, torch.from_numpy(np.array(sd[canonical(k)]))) for k in model.state_dict())


def norm(x):
    """results / get_mol() as plain values: tuples as lists, tensors and numpy scalars as numbers"""
    if isinstance(x, dict):
        return {k: norm(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [norm(v) for v in x]
    if isinstance(x, (torch.Tensor, np.ndarray)):
        return norm(x.tolist())
    if isinstance(x, np.generic):
        return x.item()
    return x


def assert_same(got, want, tol=TOL, path="results"):
    """the same structure, keys (in order), strings and integers; floats within tol (relative above 1)"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (path, got, want)
        for k in want:
            assert_same(got[k], want[k], tol, "%s[%r]" % (path, k))
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (path, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, tol, "%s[%d]" % (path, i))
    elif isinstance(want, float):
        assert isinstance(got, (int, float)) and abs(got - want) <= tol * max(1.0, abs(want)), (path, got, want)
    else:
        assert type(got) is type(want) and got == want, (path, got, want)


class DecodeGolden:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        (self.H, self.L, self.diterT, self.B, self.n_motif, self.n_attach, self.max_step, self.beam,
         self.seed) = [int(v) for v in self.z["meta"]]
        self.rnn, self.topo_bias = str(self.z["rnn"]), float(self.z["topo_bias"])
        for k in ("results", "mols", "cands", "ops", "features"):
            setattr(self, k, json.loads(str(self.z[k])))

    def vocab(self):
        from ggpm_amd.vocab import IndexPairVocab
        return IndexPairVocab(self.n_motif, self.n_attach)

    def decoder(self, device=None):
        from ggpm_amd.motif_decoder import MotifDecoder
        d = MotifDecoder(self.vocab(), AtomVocab(), self.rnn, self.H, self.H, self.L, self.diterT, 1, 0.0)
        d.load_state_dict(state_dict(d, [str(k) for k in self.z["param_names"]], self.seed, self.topo_bias), strict=True)
        d.eval()
        return d if device is None else d.to(device)

    def latents(self, device):
        return tuple(torch.from_numpy(self.z[k]).to(device) for k in ("root_vecs", "tree_vecs", "graph_vecs"))

    def tables(self):
        return {k: self.z["tree_" + k] for k in ("fnode", "fmess", "agraph", "bgraph")}

    def check(self, dec, results, mols):
        """a decode's results, molecules, tried candidates with their scores and final tree tables against the
        reference's"""
        assert_same(norm(results), self.results)
        assert norm(mols) == self.mols
        trace = [[c, s] for (_, _, _, c, s) in dec.last_decode_trace]
        assert [c for c, _ in trace] == [c for c, _ in self.cands]
        for (_, s), (_, w) in zip(trace, self.cands):
            assert_same(s, w, path="attachment scores")
        tree = dec.last_decode_tree
        tabs = self.tables()
        assert tree.n_nodes == len(tabs["fnode"]) and tree.n_edges == len(tabs["fmess"])
        for k, want in tabs.items():
            assert np.array_equal(getattr(tree, k)[:len(want)], want), k
