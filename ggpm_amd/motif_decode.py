"""Greedy decode of the tree-only decoder -- reference ggpm/decoder.py:901-1095 (``MotifDecoder.decode``) on the
library's kernels (csrc/motif_decode.hip).

Chemistry goes through a *graph batch*: an object with the methods of the reference's ``IncGraph`` that decode calls --
the constructor ``(vocab, avocab, batch_size, max_nodes=, max_edges=, node_fdim=, edge_fdim=)``, ``add_mol``,
``get_assm_cands``, ``try_add_mol``, ``get_mol`` -- plus ``anchor_label(ismiles, atom)``, the label the reference computes
inline with ``get_anchor_smiles(Chem.MolFromSmiles(ismiles), atom, ...)``.  ``ggpm_amd.synth_graph.SynthGraphBatch`` is a
synthetic one; INTEGRATION.md (*Decoding*) shows how to wrap the reference's own ``IncGraph``.  An exception the graph
batch (or the vocabulary lookup of an anchor) raises in the candidate loop ends that molecule's expansion, as the reference's
try/except (decoder.py:1037) does; nothing else is caught.

Host: the decode-time tree (:class:`DecodeTree`, IncTree without networkx), the stacks, the graph batch and the results.
Device, resident for the whole decode: the message states (h, and c for LSTM) and the tree's tables (motif ids, fmess,
agraph, bgraph), edited from uploads.  One step:
  1. upload the edits left by the previous step's assembly with the current nodes and their molecules; tree step
     (read-outs); topology head with its sigmoid; copy the probabilities back;
  2. expand / pop on the host (the tree edits); upload them with the new messages; tree step (messages); cluster heads
     and ``hier_topk`` of the expanding molecules; copy the top k back;
  3. every beam entry's candidates on the host (``get_assm_cands`` changes nothing, so all entries can be listed before
     any is tried); when some entry has several, upload them, score all in one launch, copy the scores back;
  4. assembly in the reference's order with those scores.
At most 3 uploads, 3 device-to-host copies and 12 launches per step, whatever the batch size or the beam
(``MotifDecoder.last_decode_stats`` holds the counts of every step).
"""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import functional as F_
from .decoder_heads import MAX_POS

MAX_NB = 12                                     # IncBase's max_nb
MAX_SUB_NODES = 30                              # IncTree's max_sub_nodes: the width of a cgraph row
L_TREE, L_MLP, L_TOPK, L_ASSM = 2, 2, 1, 1      # launches per library call
NO_FACTORY = ("MotifDecoder.decode needs a graph batch (the molecule-assembly object, the reference's IncGraph): pass "
              "graph_batch_factory= (ggpm_amd.synth_graph.SynthGraphBatch, or the reference's IncGraph wrapped as "
              "INTEGRATION.md, section Decoding, shows), set args.graph_batch_factory for reconstruct / "
              "PropertyVAEOptimizer.forward, or set decoder.graph_batch_factory")


class DecodeTree:
    """IncBase / IncTree of reference ggpm/inc_graph.py:10-92 with lists and numpy.  Node 0 and message 0 are the pads;
    predecessors and successors are kept in insertion order, as networkx keeps them; the tables are written slot for
    slot as IncBase.add_edge writes them.  Every table write is also queued for the device copy (``take_edits``).
    ``cgraph`` (IncTree's cluster atoms per node, ``MAX_SUB_NODES`` wide) is kept only when asked for: the tree-only
    decode never reads it.  With it, the second node column and the cgraph slots are queued as table edits 3 and 4."""

    def __init__(self, max_nodes: int, max_edges: int, max_nb: int = MAX_NB, cgraph: bool = False):
        self.max_nb = max_nb
        self.fnode = np.zeros((max_nodes, 2), np.int64)
        self.fmess = np.zeros((max_edges, 3), np.int64)
        self.agraph = np.zeros((max_nodes, max_nb), np.int64)
        self.bgraph = np.zeros((max_edges, max_nb), np.int64)
        self.cgraph = np.zeros((max_nodes, MAX_SUB_NODES), np.int64) if cgraph else None
        self.preds, self.succs = [[]], [[]]
        self.edge = {}
        self.n_edges = 1
        self.cluster, self.cluster_edges, self.attached = {}, {}, {}
        self._node_edits, self._tab_edits = {}, {}

    @property
    def n_nodes(self):
        return len(self.preds)

    def add_node(self):
        """(the reference's add_node(feature) does not store the feature: a root's row stays motif 0)"""
        self.preds.append([])
        self.succs.append([])
        return len(self.preds) - 1

    def in_degree(self, i):
        return len(self.preds[i])

    def can_expand(self, i):
        return len(self.preds[i]) < self.max_nb

    def set_node_feature(self, i, clab, ilab):
        self.fnode[i] = (clab, ilab)
        self._node_edits[i] = clab
        if self.cgraph is not None:
            self._tab_edits[(3, i, 1)] = ilab

    def _write(self, tab, table, row, slot, value):
        if not -self.max_nb <= slot < self.max_nb:
            raise IndexError("decode tree: slot %d of a %d-slot row" % (slot, self.max_nb))
        slot %= self.max_nb             # slot -1 is the last one, as the reference's tensor indexing has it
        table[row, slot] = value
        self._tab_edits[(tab, row, slot)] = value

    def add_edge(self, i, j, feature=None):
        if (i, j) in self.edge:
            return self.edge[(i, j)]
        self.preds[j].append(i)
        self.succs[i].append(j)
        idx = self.edge[(i, j)] = self.n_edges
        self.n_edges += 1
        self._write(0, self.agraph, j, len(self.preds[j]) - 1, idx)
        if feature is not None:
            self.fmess[idx] = feature
            self._tab_edits[(2, idx, 0)], self._tab_edits[(2, idx, 1)] = int(feature[0]), int(feature[2])
        for s, k in enumerate([k for k in self.preds[i] if k != j]):
            self._write(1, self.bgraph, idx, s, self.edge[(k, i)])
        for k in self.succs[j]:
            if k != i:
                self._write(1, self.bgraph, self.edge[(j, k)], len(self.preds[j]) - 2, idx)
        return idx

    def register_cgraph(self, i, nodes, edges, attached):
        if self.cgraph is not None:
            self.cgraph[i, :len(nodes)] = nodes         # (more atoms than the row holds raise, as the reference's write)
            for s, a in enumerate(nodes):
                self._tab_edits[(4, i, s)] = int(a)
        self.cluster[i], self.cluster_edges[i], self.attached[i] = nodes, edges, attached

    def update_attached(self, i, inter_label):
        if len(self.cluster[i]) > 1:
            self.attached[i].extend(list(zip(*inter_label))[0])

    def get_cluster(self, i):
        return self.cluster[i], self.cluster_edges[i], self.attached[i]

    def take_edits(self):
        """-> (node edits [(node, motif)], table edits [(0 agraph / 1 bgraph / 2 fmess / with cgraph: 3 fnode column 1,
        4 cgraph; row, slot, value)]) queued since the last call: one per node / slot, its last value (the device applies
        the edits in parallel)"""
        out = list(self._node_edits.items()), [k + (v,) for k, v in self._tab_edits.items()]
        self._node_edits, self._tab_edits = {}, {}
        return out


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _width(c):
    return len(c) if hasattr(c, "__len__") else 1


def decode(dec, mols, src_mol_vecs, greedy=True, max_decode_step=100, beam=5, graph_batch_factory=None):
    """``MotifDecoder.decode`` -> (results, graph_batch.get_mol())"""
    factory = graph_batch_factory if graph_batch_factory is not None else getattr(dec, "graph_batch_factory", None)
    if factory is None:
        raise NotImplementedError(NO_FACTORY)
    if not greedy:
        raise NotImplementedError("MotifDecoder.decode: greedy=False (sampled decoding) is not part of this build; every "
                                  "caller in the reference decodes greedily")
    if dec.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in dec.modules()):
        raise NotImplementedError("MotifDecoder.decode runs without dropout: call model.eval() first (reconstruct.py does)")
    with torch.no_grad():
        run = _Decode(dec, factory, src_mol_vecs, int(max_decode_step), int(beam))
        out = run.run()
    dec.last_decode_stats, dec.last_decode_tree, dec.last_decode_trace = run.stats, run.tree, run.trace
    return out


class _Decode:
    def __init__(self, dec, factory, src_mol_vecs, max_steps, beam):
        root = src_mol_vecs[0]
        F_._need_gpu(*src_mol_vecs)
        self.dec, self.max_steps, self.beam = dec, max_steps, beam
        self.B = B = root.shape[0]
        self.H, self.L = H, L = dec.hidden_size, dec.latent_size
        self.dev = dev = root.device
        self.vocab = dec.vocab
        self.n_cls, self.n_icls = (int(v) for v in dec.vocab.size())
        if not 1 <= beam <= min(16, self.n_cls, self.n_icls):
            raise ValueError("MotifDecoder.decode: beam %d (1 to 16 and at most the vocabulary sizes %d / %d)"
                             % (beam, self.n_cls, self.n_icls))
        self.src_root, self.src_tree, self.src_graph = (v.detach().float().contiguous() for v in src_mol_vecs)
        hmpn = dec.hmpn
        self.gb = factory(dec.vocab, dec.avocab, B, max_nodes=400, max_edges=500, node_fdim=hmpn.atom_size,
                          edge_fdim=hmpn.atom_size + hmpn.bond_size)
        self.lib = _lib.load()
        te = hmpn.tree_encoder
        rnn = te.rnn
        self.lstm = hasattr(rnn, "W_f")
        if self.lstm:
            ws = [rnn.W_i[0].weight, rnn.W_i[0].bias, rnn.W_o[0].weight, rnn.W_o[0].bias, rnn.W_f[0].weight,
                  rnn.W_f[0].bias, rnn.W[0].weight, rnn.W[0].bias]
        else:
            ws = [rnn.W_z.weight, rnn.W_z.bias, rnn.W_r.weight, rnn.U_r.weight, rnn.U_r.bias, rnn.W_h.weight, rnn.W_h.bias]
        self.params = [p.detach().contiguous() for p in [hmpn.E_c[0].weight, te.W_o[0].weight, te.W_o[0].bias] + ws]
        self.param_ptrs = (ctypes.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        self.depth = rnn.depth
        self.N = N = 2 + B + B * max_steps          # a step adds at most one node per molecule
        self.E = E = 1 + B + 3 * B * max_steps      # ... and at most three messages (expand, then a forced backtrack)
        i32 = dict(dtype=torch.int32, device=dev)
        self.fnode, self.fmess = torch.zeros(N, **i32), torch.zeros(E, 2, **i32)
        self.agraph, self.bgraph = torch.zeros(N, MAX_NB, **i32), torch.zeros(E, MAX_NB, **i32)
        self.h = torch.zeros(E, H, device=dev)
        self.c = torch.zeros(E, H, device=dev) if self.lstm else None
        ld = (H + 3) // 4 * 4
        self.node_out, self.mess_out, self.hid = (torch.empty(B, ld, device=dev) for _ in range(3))
        self.topo = torch.empty(B, device=dev)
        self.cls_out = torch.empty(B, self.n_cls, device=dev)
        self.icls_out = torch.empty(B, self.n_icls, device=dev)
        owner = getattr(self.vocab, "owner", None)
        if owner is None:       # a PairVocab: the motif whose mask row is 0 at the attachment
            owner = torch.as_tensor(self.vocab.mask).cpu().argmax(dim=0).numpy()
        self.owner = torch.from_numpy(np.asarray(owner, np.int32)).to(dev)
        self.tree = DecodeTree(N, E)
        self.stats, self.trace = [], []
        self.cur = {}

    # ------------------------------------------------------------------ device calls
    def _upload(self, lists, edits=True):
        """One host-to-device copy: the queued tree edits (when ``edits``), then ``lists`` -> (buffer, node edits, table
        edits, offset of every list)"""
        ne, te = self.tree.take_edits() if edits else ([], [])
        parts = [np.asarray(ne, np.int32).reshape(-1), np.asarray(te, np.int32).reshape(-1)] + \
            [np.asarray(x, np.int32).reshape(-1) for x in lists]
        offs = np.cumsum([0] + [p.size for p in parts]).tolist()
        buf = torch.from_numpy(np.concatenate(parts + [np.zeros(1, np.int32)])).to(self.dev)
        self.cur["h2d"] += 1
        return buf, len(ne), len(te), offs[2:]

    def _copy_back(self, t):
        t0 = time.perf_counter()
        out = t.cpu().numpy()
        self.cur["d2h"] += 1
        self.cur["wait_s"] += time.perf_counter() - t0
        return out

    def _tree_step(self, buf, n_ne, n_te, nodes_off=0, n_read=0, mess_off=0, n_mess=0):
        _lib.check(self.lib.ggpm_motif_decode_tree_step(
            int(self.lstm), self.H, MAX_POS, self.depth, self.param_ptrs, F_._p(self.fnode), F_._p(self.fmess),
            F_._p(self.agraph), F_._p(self.bgraph), self.N, self.E, F_._p(self.h), F_._p(self.c), _ptr(buf), n_ne, n_te,
            _ptr(buf, nodes_off), n_read, F_._p(self.node_out), self.node_out.stride(0), _ptr(buf, mess_off), n_mess,
            F_._p(self.mess_out), self.mess_out.stride(0), F_._stream()), "motif_decode_tree_step")
        self.cur["launches"] += L_TREE

    def _mlp(self, seq, vecs, ld_v, bidx, M, out, ld_out, sigmoid=False):
        l1, l2 = seq[0], seq[3]
        _lib.check(self.lib.ggpm_motif_decode_mlp(
            F_._p(vecs), ld_v, bidx, F_._p(self.src_tree), self.src_tree.stride(0), M, self.H, self.L, F_._p(l1.weight),
            F_._p(l1.bias), F_._p(l2.weight), F_._p(l2.bias), l2.weight.shape[0], int(sigmoid), F_._p(self.hid),
            self.hid.stride(0), F_._p(out), ld_out, F_._stream()), "motif_decode_mlp")
        self.cur["launches"] += L_MLP

    def _heads_topk(self, vecs, ld_v, bidx, M, k, root):
        """clsNN, iclsNN and hier_topk (root: the arg-max motif and its sorted masked attachments) of M rows ->
        (scores [M, k], motifs [M, k], attachments [M, k])"""
        self._mlp(self.dec.clsNN, vecs, ld_v, bidx, M, self.cls_out, self.n_cls)
        self._mlp(self.dec.iclsNN, vecs, ld_v, bidx, M, self.icls_out, self.n_icls)
        out = torch.empty(M, 3 * k, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.ggpm_hier_topk(F_._p(self.cls_out), self.n_cls, self.n_cls, F_._p(self.icls_out), self.n_icls,
                                           self.n_icls, F_._p(self.owner), M, k, int(root), F_._p(out), F_._stream()),
                   "hier_topk")
        self.cur["launches"] += L_TOPK
        out = self._copy_back(out)
        return out[:, :k].view(np.float32), out[:, k:2 * k], out[:, 2 * k:]

    def _new_counts(self):
        self.cur = {"launches": 0, "d2h": 0, "h2d": 0, "expand": 0, "scored": 0, "wait_s": 0.0}

    # ------------------------------------------------------------------ the loop
    def run(self):
        dec, B, H, vocab, gb, tree = self.dec, self.B, self.H, self.vocab, self.gb, self.tree
        results = [[] for _ in range(B)]
        stack = [[] for _ in range(B)]
        self._new_counts()
        # the root (decoder.py:916-949)
        if self.L == H:
            init = self.src_root
        else:
            init = F_.linear([self.src_root], [self.L], dec.W_root.weight, dec.W_root.bias)[:, :H]
        buf, _, _, offs = self._upload([np.arange(B)], edits=False)
        k0 = min(5, self.n_icls)
        sc, rc, ri = self._heads_topk(init, F_._ld(init), _ptr(buf, offs[0]), B, k0, root=True)
        for b in range(B):
            results[b].append({'root': vocab.get_smiles(int(rc[b, 0]))})
            results[b][-1]['top-5-root-attachments'] = [(vocab.get_ismiles(int(ri[b, q])), float(sc[b, q]))
                                                        for q in range(k0)]
        for b in range(B):
            results[b][-1]['Attaching Fragment'] = {'mol': int(rc[b, 0]), 'attachment': vocab.get_ismiles(int(ri[b, 0]))}
        super_root = tree.add_node()
        for b in range(B):
            root = tree.add_node()
            tree.add_edge(super_root, root)
            stack[b].append(root)
            new_atoms, new_bonds, attached = gb.add_mol(b, vocab.get_ismiles(int(ri[b, 0])), [], 0)
            tree.register_cgraph(root, new_atoms, new_bonds, attached)
            results[b][-1]['Attaching Fragment']['attachment-points'] = (new_atoms, attached)
        for r, mol in zip(results, gb.get_mol()):
            r[-1]['partial-graph'] = mol
        self.h[1:B + 1].copy_(init[:, :H])      # h[1:B+1] = init_vecs: the super-root messages (LSTM: the hidden half)
        self.root_stats = self.cur

        for t in range(self.max_steps):
            for r in results:
                r.append({})
            batch_list = [b for b in range(B) if stack[b]]
            if not batch_list:
                break
            self._new_counts()
            self._step(t, batch_list, stack, results)
            for mol, r in zip(gb.get_mol(), results):
                r[-1]['partial-graph'] = mol
            self.stats.append(self.cur)
        return results, gb.get_mol()

    def _step(self, t, batch_list, stack, results):
        tree, vocab = self.tree, self.vocab
        n = len(batch_list)
        # 1. read-outs of the current nodes, the topology head (decoder.py:963-976)
        buf, n_ne, n_te, offs = self._upload([[stack[b][-1] for b in batch_list], batch_list])
        self._tree_step(buf, n_ne, n_te, nodes_off=offs[0], n_read=n)
        self._mlp(self.dec.topoNN, self.node_out, self.node_out.stride(0), _ptr(buf, offs[1]), n, self.topo, 1,
                  sigmoid=True)
        topo = self._copy_back(self.topo[:n])
        # 2. expand or pop (decoder.py:978-998), the new messages, the cluster heads of the expanding molecules
        new_mess, expand = [], []
        for i, bid in enumerate(batch_list):
            p = float(topo[i])
            results[bid][-1]['Generate fragment'] = p
            if p > 0.5 and tree.can_expand(stack[bid][-1]):
                expand.append((len(new_mess), bid))
                new_node = tree.add_node()
                new_mess.append(tree.add_edge(stack[bid][-1], new_node, (stack[bid][-1], new_node, 0)))
                stack[bid].append(new_node)
            else:
                child = stack[bid].pop()
                if stack[bid]:
                    nth = tree.in_degree(stack[bid][-1])
                    new_mess.append(tree.add_edge(child, stack[bid][-1], (child, stack[bid][-1], nth)))
        self._check_independent(new_mess)
        rows = {i: q for q, (i, _) in enumerate(expand)}
        expanding = [bid for _, bid in expand]
        buf, n_ne, n_te, offs = self._upload([[(e, rows.get(i, -1)) for i, e in enumerate(new_mess)], expanding])
        self._tree_step(buf, n_ne, n_te, mess_off=offs[0], n_mess=len(new_mess))
        if not expanding:
            return
        self.cur["expand"] = 1
        scores, cls_topk, icls_topk = self._heads_topk(self.mess_out, self.mess_out.stride(0), _ptr(buf, offs[1]),
                                                       len(expanding), self.beam, root=False)
        # 3. every beam entry's candidates; the entries with several scored in one launch
        plans, meta, ids = [], [], []
        n_cand = 0
        for i, bid in enumerate(expanding):
            fa_node = stack[bid][-2]
            fa_cluster, _, fa_used = tree.get_cluster(fa_node)
            results[bid][-1]['top-5-inter-cands'] = [(vocab.get_smiles(int(x)), vocab.get_ismiles(int(y)), float(s))
                                                     for x, y, s in zip(cls_topk[i], icls_topk[i], scores[i])]
            entries = []
            for kk in range(self.beam):
                clab, ilab = int(cls_topk[i][kk]), int(icls_topk[i][kk])
                smiles, ismiles = vocab.get_smiles(clab), vocab.get_ismiles(ilab)
                try:
                    inter_cands, anchor_smiles, attach_points = self.gb.get_assm_cands(fa_cluster, fa_used, ismiles)
                    icls = [vocab[(smiles, x)][1] for x in anchor_smiles] if len(inter_cands) > 1 else None
                except Exception:       # the reference's try/except (decoder.py:1037): the expansion fails here
                    entries.append((clab, ilab, None))
                    break
                slot = nth = None
                if len(inter_cands) > 1:
                    cands = inter_cands if len(attach_points) <= 2 else [(x[0], x[-1]) for x in inter_cands]
                    k = len(icls)
                    nth = tree.in_degree(fa_node)
                    if k not in (1, 2) or any(_width(c) != k for c in cands) or \
                            not all(0 <= int(x) < self.n_icls for x in icls) or nth >= MAX_POS:
                        # enum_attach / get_assm_score raise on these in the reference (row counts differ, an
                        # embedding or onehot index out of range): the expansion fails here
                        entries.append((clab, ilab, None))
                        break
                    meta.append((len(cands), k, nth, bid, n_cand, len(ids)))
                    ids.extend(int(x) for x in icls)
                    slot = n_cand
                    n_cand += len(cands)
                entries.append((clab, ilab, (ismiles, inter_cands, attach_points, nth, slot)))
            plans.append(entries)
        assm = None
        if meta:
            self.cur["scored"] = 1
            buf, _, _, offs = self._upload([meta, ids], edits=False)
            score = torch.empty(n_cand, device=self.dev)
            l1, wa = self.dec.matchNN[0], self.dec.W_assm
            _lib.check(self.lib.ggpm_motif_decode_assm_score(
                F_._p(self.dec.E_assm[0].weight), self.n_icls, self.H, self.L, _ptr(buf, offs[0]), _ptr(buf, offs[1]),
                len(meta),
                F_._p(l1.weight), l1.weight.stride(0), F_._p(l1.bias), F_._p(wa.weight), F_._p(wa.bias),
                F_._p(self.src_graph), self.src_graph.stride(0), F_._p(score), F_._stream()), "motif_decode_assm_score")
            self.cur["launches"] += L_ASSM
            assm = self._copy_back(score)
            if np.isnan(assm).any():
                raise RuntimeError("MotifDecoder.decode: the attachment-score kernel refused a candidate table row")
        # 4. assembly (decoder.py:1037-1087) and the forced backtrack (:1089-1099)
        for i, bid in enumerate(expanding):
            new_node, fa_node = stack[bid][-1], stack[bid][-2]
            success = False
            for kk, (clab, ilab, ent) in enumerate(plans[i]):
                tree.set_node_feature(new_node, clab, ilab)       # (kept when the entry fails, as the reference's is)
                if ent is None:
                    break
                ismiles, inter_cands, attach_points, nth, slot = ent
                if len(inter_cands) == 0:
                    self.trace.append((t, bid, kk, [], []))
                    continue
                if len(inter_cands) == 1:
                    sc, sorted_cands, nth_child = [], [(inter_cands[0], 0)], 0
                else:
                    sc = [float(v) for v in assm[slot:slot + len(inter_cands)]]
                    sorted_cands, nth_child = sorted(zip(inter_cands, sc), key=lambda x: x[1], reverse=True), nth
                self.trace.append((t, bid, kk, [list(c) for c in inter_cands], sc))
                done, success = self._attach(bid, ismiles, sorted_cands, attach_points, nth_child, new_node, fa_node,
                                             results)
                if done:
                    break
            if not success:
                child = stack[bid].pop()
                nth = tree.in_degree(stack[bid][-1])
                tree.add_edge(child, stack[bid][-1], (child, stack[bid][-1], nth))
                child = stack[bid].pop()
                if stack[bid]:
                    nth = tree.in_degree(stack[bid][-1])
                    tree.add_edge(child, stack[bid][-1], (child, stack[bid][-1], nth))

    def _attach(self, bid, ismiles, sorted_cands, attach_points, nth_child, new_node, fa_node, results):
        """the candidates of one beam entry in order -> (the beam loop ends, success)"""
        gb, tree = self.gb, self.tree
        for cand, _ in sorted_cands:
            inter_label = list(zip(cand, attach_points))
            try:
                if not gb.try_add_mol(bid, ismiles, inter_label):
                    continue
                new_atoms, new_bonds, attached = gb.add_mol(bid, ismiles, inter_label, nth_child)
            except Exception:           # the reference's try/except: the expansion fails
                return True, False
            tree.register_cgraph(new_node, new_atoms, new_bonds, attached)
            tree.update_attached(fa_node, inter_label)
            try:
                anchors = [gb.anchor_label(ismiles, a) for a in attach_points]
            except Exception:
                return True, False
            results[bid][-1]['Attaching Fragment'] = (ismiles, attach_points, inter_label, anchors)
            return True, True
        return False, False

    def _check_independent(self, new_mess):
        """The message kernel runs every new message in its own workgroup, so none may read another of the same step.
        Holds for the decode tree: a step adds one message per molecule before its message update."""
        if len(new_mess) > 1:
            s = set(new_mess)
            if any(int(v) in s for v in self.tree.bgraph[new_mess].reshape(-1) if v):
                raise RuntimeError("MotifDecoder.decode: a new message reads another message of the same step")
