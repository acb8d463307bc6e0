#!/usr/bin/env python3
"""Golden fixtures of the hierarchical decoder's greedy decode, produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_hier_decode.py      (build container only; needs the reference checkout)

Per case the reference's own ``HierMPNDecoder.decode`` (ggpm/decoder.py:303-472) runs on CPU with seeded parameters
(``params.seeded_state_dict`` over its parameter list, the topology head's output bias raised by ``topo_bias``) and
seeded latents.  ``ggpm.decoder.IncGraph`` is replaced by ``RefTables`` below: the fragment rules of
``ggpm_amd.synth_graph.SynthGraphBatch`` with the atom tables kept by the reference's own ``IncBase`` -- every node and
message goes through ``IncBase.add_node`` / ``IncBase.add_edge`` -- so that the recorded tables pin
``SynthHierGraphBatch``'s restatement of them and not that restatement itself.  ``get_anchor_smiles`` and
``Chem.MolFromSmiles`` are stand-ins returning the synthetic anchor labels.  The reference's hierarchical decode catches
nothing; a case in which anything raised is refused (the exception ends the run).

Recorded per case: the results and get_mol() (JSON), the candidate list and attachment scores of every beam entry tried,
the tree operations (``register_cgraph`` included) and the ``add_mol`` calls in order, the final tree tables with cgraph
and the final atom tables, the branches the case reaches, and the smallest decision margin (topology probability against
0.5, the gaps of every top-k selection, the gaps between distinct attachment scores); a seed whose margin is below 1e-4
is skipped.  Fixtures are DATA; no reference source text is stored.
"""
import json
import os
import sys
import types
from collections import OrderedDict, defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_decode as md  # noqa: E402

import torch  # noqa: E402

from ggpm_amd.params import seeded_state_dict  # noqa: E402
from ggpm_amd.synth_graph import SynthGraphBatch, anchor_label, fragment  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

OUT = os.path.join(HERE, "hier_decode")
MARGIN = md.MARGIN
BEAM = 5
CASES = [
    # name, rnn, H, latent, diterT, diterG, B, n_motif, max_decode_step, topo_bias, first seed, branches it must reach
    ("gru_h16_g3", "GRU", 16, 8, 1, 3, 3, 12, 25, 0.3, 100, ("several_candidates", "distinct_scores")),
    ("lstm_h16_g3", "LSTM", 16, 8, 1, 3, 3, 12, 25, 0.3, 200, ("several_candidates", "forced_backtrack")),
    ("gru_h20_t2_g1", "GRU", 20, 20, 2, 1, 4, 12, 30, 0.3, 300, ("several_candidates", "early_empty")),
    ("lstm_h24_t2_g3", "LSTM", 24, 12, 2, 3, 3, 12, 30, 0.3, 400, ("two_atom_attachments", "refusals")),
    ("gru_cap_g1", "GRU", 16, 8, 1, 1, 3, 12, 6, 2.0, 500, ("stopped_at_max",)),
]
BRANCHES = ("several_candidates", "distinct_scores", "no_candidate", "refusals", "forced_backtrack", "early_empty",
            "stopped_at_max", "two_atom_attachments")
norm, gaps, lsm = md.norm, md.gaps, md.lsm


def make_graph_class(IncBase, avocab, rec):
    n_bond, max_pos = 4, 20

    class RefTables(SynthGraphBatch):
        def __init__(self, vocab, avocab_, batch_size, node_fdim, edge_fdim, max_nodes=100, max_edges=300, max_nb=10):
            SynthGraphBatch.__init__(self, vocab, avocab_, batch_size, max_nodes, max_edges, node_fdim, edge_fdim, max_nb)
            self.base = IncBase(batch_size, node_fdim, edge_fdim, max_nodes, max_edges, max_nb)
            self.base.fnode, self.base.fmess = self.base.fnode.float(), self.base.fmess.float()
            rec["graphs"].append(self)

        def get_tensors(self):
            b = self.base
            return b.fnode, b.fmess, b.agraph, b.bgraph, None

        def _atom(self, symbol):
            f = torch.zeros(avocab.size())
            f[avocab[(symbol, 0)]] = 1
            return f

        def _mess(self, symbol, btype, nth):
            f1, f2, f3 = torch.zeros(avocab.size()), torch.zeros(n_bond), torch.zeros(max_pos)
            f1[avocab[(symbol, 0)]] = 1
            f2[btype] = 1
            f3[nth] = 1
            return torch.cat([f1, f2, f3])

        def get_assm_cands(self, *a):
            out = SynthGraphBatch.get_assm_cands(self, *a)
            rec["cands"].append([[list(c) for c in out[0]], []])
            return out

        def try_add_mol(self, *a):
            ok = SynthGraphBatch.try_add_mol(self, *a)
            rec["refused"] += not ok
            return ok

        def add_mol(self, bid, ismiles, inter_label, nth_child):
            size, labels, _ = fragment(ismiles)
            amap = {int(y): int(x) for x, y in inter_label}
            new_atoms, attached = [], []
            for i in range(size):
                if i in amap:
                    new_atoms.append(amap[i])
                    attached.append(amap[i])
                    continue
                idx = self.base.add_node(self._atom(labels[i]))
                self.label.append(labels[i])
                self.degree.append(0)
                self.owner.append(bid)
                assert idx == len(self.label) - 1
                amap[i] = idx
                new_atoms.append(idx)
                self.batch[bid].append(idx)
            btype = 0 if size == 2 else 1
            pairs = [(i, i + 1) for i in range(size - 1)] + ([(size - 1, 0)] if size > 2 else [])
            new_bonds = []
            for p, q in pairs:
                a1, a2 = amap[p], amap[q]
                if (min(a1, a2), max(a1, a2)) not in self.bonds:
                    self._bond(a1, a2)
                    self.base.add_edge(a1, a2, self._mess(labels[p], btype, nth_child if a2 in attached else 0))
                    self.base.add_edge(a2, a1, self._mess(labels[q], btype, nth_child if a1 in attached else 0))
                new_bonds.extend([self.base.edge_dict[(a1, a2)], self.base.edge_dict[(a2, a1)]])
            self._mol.pop(bid, None)
            out = new_atoms, new_bonds, [amap[p] for p in sorted(int(y) for _, y in inter_label)]
            rec["add_mol"].append([int(bid), str(ismiles), [[int(x), int(y)] for x, y in inter_label], int(nth_child),
                                   [list(map(int, o)) for o in out]])
            return out
    return RefTables


def run_case(D, IG, base_tree, rnn, H, L, dT, dG, B, n_motif, max_step, bias, seed):
    from ggpm.vocab import common_atom_vocab
    n_attach = 3 * n_motif
    vocab = IndexPairVocab(n_motif, n_attach)
    torch.manual_seed(seed)
    model = D.HierMPNDecoder(vocab, common_atom_vocab, rnn, H, H, L, dT, dG, 0.0)
    model.eval()
    names = [k for k, _ in model.named_parameters()]
    sd = seeded_state_dict(OrderedDict((k, tuple(p.shape)) for k, p in model.named_parameters()), seed)
    sd["topoNN.3.bias"] = sd["topoNN.3.bias"] + np.float32(bias)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(sd[k]))
    rec = {"cls": [], "cands": [], "ops": [], "feat": defaultdict(int), "registered": set(), "refused": 0, "trees": [],
           "graphs": [], "add_mol": []}
    real_cls, real_assm = model.get_cls_score, model.get_assm_score

    def cls_spy(src, bidx, vecs, labs):
        c, i = real_cls(src, bidx, vecs, labs)
        rec["cls"].append((c.detach().numpy().copy(), i.detach().numpy().copy()))
        return c, i

    def assm_spy(*a):
        s = real_assm(*a)
        rec["cands"][-1][1] = [float(v) for v in s.tolist()]
        return s
    model.get_cls_score, model.get_assm_score = cls_spy, assm_spy

    class Tree(base_tree):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            rec["trees"].append(self)

        def add_node(self, feature=None):
            rec["ops"].append(["node"])
            return super().add_node(feature)

        def add_edge(self, i, j, feature=None):
            rec["ops"].append(["edge", int(i), int(j), None if feature is None else [int(v) for v in feature]])
            return super().add_edge(i, j, feature)

        def set_node_feature(self, idx, feature):
            rec["ops"].append(["feat", int(idx)] + [int(v) for v in feature])
            rec["feat"][int(idx)] += 1
            return super().set_node_feature(idx, feature)

        def register_cgraph(self, i, nodes, edges, attached):
            rec["registered"].add(int(i))
            rec["ops"].append(["cgraph", int(i), [int(v) for v in nodes], [int(v) for v in edges],
                               [int(v) for v in attached]])
            return super().register_cgraph(i, nodes, edges, attached)

    D.IncTree, D.IncGraph = Tree, make_graph_class(IG.IncBase, common_atom_vocab, rec)
    D.Chem = types.SimpleNamespace(MolFromSmiles=lambda s: s)
    D.get_anchor_smiles = lambda mol, a, fn: anchor_label(mol, a)
    rs = np.random.RandomState(seed + 7)
    vecs = [rs.standard_normal((B, L)).astype(np.float32) for _ in range(3)]
    try:
        with torch.no_grad():
            results, mols = model.decode(None, tuple(torch.from_numpy(v) for v in vecs), greedy=True,
                                         max_decode_step=max_step, beam=BEAM)
    except Exception as e:  # noqa: BLE001  (the reference catches nothing: a case in which anything raised is refused)
        return None, "raised %r" % e
    failed = [n for n in rec["feat"] if n not in rec["registered"]]
    res = norm(results)
    margins = [abs(e["Generate fragment"] - 0.5) for r in res for e in r[1:] if "Generate fragment" in e]
    owner, mask = vocab.owner, vocab.mask.numpy()
    k0 = min(5, n_attach)
    for crow, irow in zip(*rec["cls"][0]):
        margins += gaps(crow, 1)
        margins += gaps(irow + mask[int(np.argmax(crow))], k0)
    for c, i in rec["cls"][1:]:
        for crow, irow in zip(c, i):
            lc = lsm(crow)
            margins += gaps(lc, BEAM)
            sums = []
            for m in np.argsort(-lc, kind="stable")[:BEAM]:
                li = lsm(irow + mask[m])
                own = li[owner == m]
                margins += gaps(own, len(own) - 1)
                sums += list(lc[m] + np.sort(li)[::-1][:BEAM])
            margins += gaps(sums, BEAM)
    for _, scores in rec["cands"]:
        if len(scores) > 1 and max(scores) != min(scores):
            margins += [g for g in gaps(scores, len(scores) - 1) if g > 0]
    margin = float(min(margins)) if margins else 1.0
    active = [sum(1 for e in r if "Generate fragment" in e) for r in res]
    feats = {
        "several_candidates": any(len(c) > 1 for c, _ in rec["cands"]),
        "distinct_scores": any(len(set(s)) > 1 for _, s in rec["cands"]),
        "no_candidate": any(len(c) == 0 for c, _ in rec["cands"]),
        "refusals": rec["refused"] > 0,
        "forced_backtrack": len(failed) > 0,
        "early_empty": min(active) < max(active),
        "stopped_at_max": any("Generate fragment" in r[-1] for r in res),
        "two_atom_attachments": any(len(c) > 1 and len(c[0]) == 2 for c, _ in rec["cands"]),
    }
    tree, graph = rec["trees"][0], rec["graphs"][0].base
    n_nodes, n_edges = len(tree.graph), len(tree.edge_dict)
    na, ea = len(graph.graph), len(graph.edge_dict)
    out = {
        "meta": np.array([H, L, dT, dG, B, n_motif, n_attach, max_step, BEAM, seed], np.int64),
        "rnn": np.array(rnn), "topo_bias": np.array(bias, np.float64), "param_names": np.array(names),
        "root_vecs": vecs[0], "tree_vecs": vecs[1], "graph_vecs": vecs[2],
        "results": np.array(json.dumps(res)), "mols": np.array(json.dumps(norm(mols))),
        "cands": np.array(json.dumps(rec["cands"])), "ops": np.array(json.dumps(rec["ops"])),
        "add_mol": np.array(json.dumps(rec["add_mol"])),
        "features": np.array(json.dumps(feats)), "margin": np.array(margin),
        "tree_fnode": tree.fnode[:n_nodes].numpy().astype(np.int32),
        "tree_fmess": tree.fmess[:n_edges].numpy().astype(np.int32),
        "tree_agraph": tree.agraph[:n_nodes].numpy().astype(np.int32),
        "tree_bgraph": tree.bgraph[:n_edges].numpy().astype(np.int32),
        "tree_cgraph": tree.cgraph[:n_nodes].numpy().astype(np.int32),
        "atom_fnode": graph.fnode[:na].numpy().astype(np.float32),
        "atom_fmess": graph.fmess[:ea].numpy().astype(np.float32),
        "atom_agraph": graph.agraph[:na].numpy().astype(np.int32),
        "atom_bgraph": graph.bgraph[:ea].numpy().astype(np.int32),
    }
    if margin < MARGIN:
        return None, "margin %.2e" % margin
    return out, feats


def main():
    mg.import_reference()
    import ggpm.decoder as D
    import ggpm.inc_graph as IG
    base_tree = D.IncTree
    os.makedirs(OUT, exist_ok=True)
    seen = defaultdict(bool)
    for (name, rnn, H, L, dT, dG, B, n_motif, max_step, bias, seed0, need) in CASES:
        for seed in range(seed0, seed0 + 300):
            out, info = run_case(D, IG, base_tree, rnn, H, L, dT, dG, B, n_motif, max_step, bias, seed)
            if out is None or not all(info[k] for k in need):
                continue
            break
        else:
            raise RuntimeError("no seed for %s" % name)
        for k, v in info.items():
            seen[k] |= v
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-14s seed=%d margin=%.2e nodes=%d atoms=%d %s -> %.1f KB" % (
            name, seed, float(out["margin"]), len(out["tree_fnode"]), len(out["atom_fnode"]),
            sorted(k for k, v in info.items() if v), os.path.getsize(path) / 1024))
    missing = [k for k in BRANCHES if not seen[k]]
    assert not missing, missing


if __name__ == "__main__":
    main()
