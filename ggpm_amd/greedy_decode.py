"""The greedy decode loop of both decoders -- reference ggpm/decoder.py:901-1095 (``MotifDecoder.decode``) and :303-472
(``HierMPNDecoder.decode``) -- with what their device backends share.  ``ggpm_amd.motif_decode`` and
``ggpm_amd.hier_decode`` each hold one subclass of :class:`GreedyDecode` (the differences between the two decoders, as
switches and hooks) and one of :class:`DeviceBackend` (their kernels).

Chemistry goes through a *graph batch*: an object with the methods of the reference's ``IncGraph`` that decode calls --
``add_mol`` (returning the fragment's atoms, its directed message ids and the parent atoms it shares),
``get_assm_cands``, ``try_add_mol``, ``get_mol`` -- plus ``anchor_label(ismiles, atom)``, the label the reference computes
inline with ``get_anchor_smiles(Chem.MolFromSmiles(ismiles), atom, ...)``.  INTEGRATION.md (*Decoding*) shows how to wrap
the reference's own ``IncGraph``.

Host: the decode-time tree (:class:`DecodeTree`, IncTree without networkx), the stacks, the graph batch and the results.
Device (the *backend*: ``root(k0)``, ``phase1``, ``phase2``, ``phase3``, ``new_counts()``, ``cur``): the message states
and the tables, resident for the whole decode and edited from uploads.  One step:
  1. ``phase1``: the tree edits left by the previous step's assembly (quads, ``_tree_edits``), the current nodes and
     their molecules, and what ``_atom_inputs`` adds; read-outs, the topology head with its sigmoid; the probabilities
     come back;
  2. expand / pop on the host (the tree edits); ``phase2``: the edits and the new messages; the message update, the
     cluster heads and ``hier_topk`` of the expanding molecules; the top k come back;
  3. every beam entry's candidates on the host (``get_assm_cands`` changes nothing, so all entries can be listed before
     any is tried).  What raises here is kept with its entry.  When some entry has several candidates, ``phase3`` scores
     all in one launch and the scores come back;
  4. assembly in the reference's order with those scores, then the forced backtrack of the molecules that attached
     nothing.  An entry that kept an exception raises it here, or is the failed expansion (``CAUGHT``).
At most 3 uploads and 3 device-to-host copies per step, and a number of launches that depends on the phases run only,
whatever the batch size or the beam (``last_decode_stats`` of the decoder holds the counts of every step).

Sampled mode (``decode_sampled``, the reference's ``greedy=False``): with a :class:`Sampling` the loop
takes the topology decision from a Bernoulli draw and tries the beam entries in an order drawn without replacement.  The
draws come from a seeded counter-based stream keyed by the molecules' sample ids: the device backend launches one draw
behind the sigmoid head and one behind ``hier_topk`` and each comes back in the copy of the values it was drawn from
(``topo_draws``, ``beam_order``), or a host ``sampler`` (a test seam) makes them from those values.  The greedy path and
its calls to the backend are the same with and without this mode.
"""
from __future__ import annotations

import ctypes
import time
from itertools import chain

import numpy as np
import torch

from . import _lib
from . import functional as F_
from .decoder_heads import MAX_POS, check_no_dropout

MAX_NB = 12                                     # IncBase's max_nb
MAX_SUB_NODES = 30                              # IncTree's max_sub_nodes: the width of a cgraph row
L_MLP, L_TOPK, L_ASSM, L_DRAW = 2, 1, 1, 1       # launches per library call


def no_factory(name, synth, optimizer):
    return ("%s.decode needs a graph batch (the molecule-assembly object, the reference's IncGraph): pass "
            "graph_batch_factory= (ggpm_amd.synth_graph.%s, or the reference's IncGraph wrapped as "
            "INTEGRATION.md, section Decoding, shows), set args.graph_batch_factory for reconstruct / "
            "%s.forward, or set decoder.graph_batch_factory" % (name, synth, optimizer))


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


def check_beam(name, dec, beam):
    n_cls, n_icls = (int(v) for v in dec.vocab.size())
    if not 1 <= beam <= min(16, n_cls, n_icls):
        raise ValueError("%s.decode: beam %d (1 to 16 and at most the vocabulary sizes %d / %d)"
                         % (name, beam, n_cls, n_icls))


def _check_eval(run_cls, dec, what):
    check_no_dropout(dec, "%s.%s runs without dropout: call model.eval() first (reconstruct.py does)" % (run_cls.NAME, what))


def _run(run_cls, dec, src_mol_vecs, max_decode_step, beam, factory, backend, sampling):
    with torch.no_grad():
        run = run_cls(dec, factory, src_mol_vecs, int(max_decode_step), int(beam), backend, sampling)
        out = run.run()
    dec.last_decode_stats, dec.last_decode_tree, dec.last_decode_trace = run.stats, run.tree, run.trace
    return out


def _factory(run_cls, dec, graph_batch_factory):
    factory = graph_batch_factory if graph_batch_factory is not None else getattr(dec, "graph_batch_factory", None)
    if factory is None:
        raise NotImplementedError(run_cls.NO_FACTORY)
    return factory


def decode(run_cls, dec, src_mol_vecs, greedy, max_decode_step, beam, graph_batch_factory, backend):
    """the ``decode`` of ``run_cls``'s decoder -> (results, graph_batch.get_mol())"""
    name = run_cls.NAME
    factory = _factory(run_cls, dec, graph_batch_factory)
    if not greedy:
        raise NotImplementedError("%s.decode: greedy=False (sampled decoding) draws from a seeded stream here, not from "
                                  "torch's global generator, and has its own entry point: call %s.decode_sampled(mols, "
                                  "src_mol_vecs, seed=...)" % (name, name))
    _check_eval(run_cls, dec, "decode")
    return _run(run_cls, dec, src_mol_vecs, max_decode_step, beam, factory, backend, None)


def decode_sampled(run_cls, dec, src_mol_vecs, seed, sample_ids, max_decode_step, beam, graph_batch_factory, backend,
                   sampler):
    """the ``decode_sampled`` of ``run_cls``'s decoder -> (results, graph_batch.get_mol())"""
    factory = _factory(run_cls, dec, graph_batch_factory)
    _check_eval(run_cls, dec, "decode_sampled")
    sampling = Sampling(seed, sample_ids, src_mol_vecs[0].shape[0], sampler)
    return _run(run_cls, dec, src_mol_vecs, max_decode_step, beam, factory, backend, sampling)


def split_seed(seed):
    """``seed`` -> (seed_lo, seed_hi), the two 32-bit halves of its low 64 bits; ``None`` takes 64 bits from torch's default
    CPU generator (``torch.manual_seed`` makes the run reproducible)"""
    if seed is None:
        lo, hi = (int(v) for v in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
        return lo, hi
    seed = int(seed) & ((1 << 64) - 1)
    return seed & 0xFFFFFFFF, seed >> 32


class Sampling:
    """What makes a decode a sampled one: the seed halves, the molecules' sample ids (the stream keys, their low 32 bits)
    and the host ``sampler`` of the test seam (``None``: the backend draws on the device)."""

    def __init__(self, seed, sample_ids, B, sampler=None):
        self.seed_lo, self.seed_hi = split_seed(seed)
        ids = np.arange(B) if sample_ids is None else np.asarray(
            sample_ids.cpu() if isinstance(sample_ids, torch.Tensor) else sample_ids)
        if ids.shape != (B,) or ids.dtype.kind not in "iu":
            raise ValueError("decode_sampled: sample_ids must be %d integers, one per molecule" % B)
        self.ids = (ids.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        self.sampler = sampler


class GreedyDecode:
    """One decode: the host loop.  A decoder's subclass names itself, sets the two switches and builds the graph batch,
    the tree and the backend in ``_setup``."""

    NAME = NO_FACTORY = None
    CAUGHT = ()                     # error policy: what the reference's try/except catches in the candidate loop, where
    #                                 it has one (decoder.py:1037); the entry that raised is then the failed expansion
    ROOT_ATTACHMENT_POINTS = False  # the root entry of the results carries 'attachment-points'

    def __init__(self, dec, factory, src_mol_vecs, max_steps, beam, backend=None, sampling=None):
        self.dec, self.max_steps, self.beam = dec, max_steps, beam
        self.sampling = sampling        # None: greedy
        self.B = src_mol_vecs[0].shape[0]
        self.vocab = dec.vocab
        self.n_cls, self.n_icls = (int(v) for v in dec.vocab.size())
        self.atab = self.NA = None      # the atom tables and their rows, where the backend has an atom level
        self._setup(factory, src_mol_vecs, backend)
        self.stats, self.trace = [], []

    # ------------------------------------------------------------------ what a decoder defines
    def _setup(self, factory, src_mol_vecs, backend):
        """the limits (``check_beam`` first, before anything is built); ``self.gb`` (the graph batch), ``self.tree``,
        ``self.be`` (``backend`` or the HIP one), and with an atom level ``self.atab`` and ``self.NA``"""
        raise NotImplementedError

    def _atom_inputs(self, nodes):
        """phase 1's atom level -> (atom-table edits, the messages and the atoms of the current nodes' clusters)"""
        return (), (), ()

    # ------------------------------------------------------------------ the loop
    def _tree_edits(self):
        """the queued tree edits as quads (0 agraph / 1 bgraph / 2 fmess / 3 fnode / 4 cgraph, row, slot, value), the
        nodes' motifs (3, node, 0, motif) first"""
        ne, te = self.tree.take_edits()
        rows = [(3, n, 0, v) for n, v in ne] + te
        return np.fromiter(chain.from_iterable(rows), np.int32, 4 * len(rows)).reshape(-1, 4)

    def _add_mol(self, *a):
        out = self.gb.add_mol(*a)
        if self.atab is not None:
            self.atab.note(out[0], out[1])
        return out

    def run(self):
        B, vocab, gb, tree = self.B, self.vocab, self.gb, self.tree
        results = [[] for _ in range(B)]
        stack = [[] for _ in range(B)]
        # the root (decoder.py:916-949, :313-350): the arg-max in both modes
        device_draws = self.sampling is not None and self.sampling.sampler is None
        if device_draws:
            if not hasattr(self.be, "start_sampling"):
                raise TypeError("%s.decode_sampled: this backend draws nothing itself: pass sampler=" % self.NAME)
            self.be.start_sampling(self.sampling)
        k0 = min(5, self.n_icls)
        sc, rc, ri = self.be.root(k0)
        for b in range(B):
            results[b].append({'root': vocab.get_smiles(int(rc[b, 0]))})
            results[b][-1]['top-5-root-attachments'] = [(vocab.get_ismiles(int(ri[b, q])), float(sc[b, q]))
                                                        for q in range(k0)]
        for b in range(B):
            results[b][-1]['Attaching Fragment'] = {'mol': int(rc[b, 0]), 'attachment': vocab.get_ismiles(int(ri[b, 0]))}
        super_root = tree.add_node()
        for b in range(B):
            root = tree.add_node()      # (add_node(feature) drops the feature: the root's row stays (0, 0))
            tree.add_edge(super_root, root)
            stack[b].append(root)
            new_atoms, new_bonds, attached = self._add_mol(b, vocab.get_ismiles(int(ri[b, 0])), [], 0)
            tree.register_cgraph(root, new_atoms, new_bonds, attached)
            if self.ROOT_ATTACHMENT_POINTS:
                results[b][-1]['Attaching Fragment']['attachment-points'] = (new_atoms, attached)
        for r, mol in zip(results, gb.get_mol()):
            r[-1]['partial-graph'] = mol
        self.root_stats = self.be.cur

        for t in range(self.max_steps):
            for r in results:
                r.append({})
            batch_list = [b for b in range(B) if stack[b]]
            if not batch_list:
                break
            self.cur = self.be.new_counts()
            if device_draws:
                self.be.step = t
            self._step(t, batch_list, stack, results)
            for mol, r in zip(gb.get_mol(), results):
                r[-1]['partial-graph'] = mol
            self.stats.append(self.cur)
        return results, gb.get_mol()

    def _step(self, t, batch_list, stack, results):
        tree, vocab = self.tree, self.vocab
        # 1. read-outs of the current nodes, the topology head (decoder.py:963-976, :361-370)
        nodes = [stack[b][-1] for b in batch_list]
        aedits, edges, atoms = self._atom_inputs(nodes)
        topo = self.be.phase1(self._tree_edits(), aedits, edges, atoms, nodes, batch_list)
        if self.sampling is not None:       # torch.bernoulli (decoder.py:374, :987): the entry records the draw
            topo = self._topo_draws(t, batch_list, topo)
        # 2. expand or pop (:978-998, :376-394), the new messages, the cluster heads of the expanding molecules
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
        self.cur["mess"] = int(bool(new_mess))      # (none: every live molecule popped its root)
        rows = {i: q for q, (i, _) in enumerate(expand)}
        expanding = [bid for _, bid in expand]
        top = self.be.phase2(self._tree_edits(), nodes, [(e, rows.get(i, -1)) for i, e in enumerate(new_mess)],
                             expanding, self.beam)
        if not expanding:
            return
        self.cur["expand"] = 1
        scores, cls_topk, icls_topk = top
        order = None
        if self.sampling is not None:       # torch.multinomial over exp(scores) (decoder.py:409-416, :1024-1033)
            log_scores = np.asarray(scores, np.float64)
            scores = np.exp(log_scores)
            order = self._beam_orders(t, expanding, scores, log_scores)
        # 3. every beam entry's candidates; the entries with several scored in one launch
        plans, meta, ids, cand_atoms = [], [], [], []
        n_cand = 0
        for i, bid in enumerate(expanding):
            fa_node = stack[bid][-2]
            fa_cluster, _, fa_used = tree.get_cluster(fa_node)
            results[bid][-1]['top-5-inter-cands'] = [(vocab.get_smiles(int(x)), vocab.get_ismiles(int(y)), float(s))
                                                     for x, y, s in zip(cls_topk[i], icls_topk[i], scores[i])]
            entries = []
            for kk in (range(self.beam) if order is None else order[i]):
                clab, ilab = int(cls_topk[i][kk]), int(icls_topk[i][kk])
                try:
                    ent = self._plan(bid, clab, ilab, fa_node, fa_cluster, fa_used, meta, ids, cand_atoms, n_cand)
                except Exception as e:      # noqa: BLE001  (met again in the assembly, if it gets there)
                    entries.append((kk, clab, ilab, e))
                    break
                if ent[4] is not None:
                    n_cand += len(ent[1])
                entries.append((kk, clab, ilab, ent))
            plans.append(entries)
        assm = None
        if meta:
            self.cur["scored"] = 1
            assm = self.be.phase3(np.asarray(meta, np.int32), ids, cand_atoms, n_cand)
            if np.isnan(assm).any():
                raise RuntimeError("%s.decode: the attachment-score kernel refused a candidate table row" % self.NAME)
        # 4. assembly (:1037-1087, :413-454) and the forced backtrack (:1089-1099, :456-466)
        for i, bid in enumerate(expanding):
            new_node, fa_node = stack[bid][-1], stack[bid][-2]
            success = False
            for kk, clab, ilab, ent in plans[i]:     # (kk: the entry's place in the top k, whatever order it is tried in)
                tree.set_node_feature(new_node, clab, ilab)       # (kept when the entry fails, as the reference's is)
                if isinstance(ent, Exception):
                    if not isinstance(ent, self.CAUGHT):
                        raise ent
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

    def _topo_draws(self, t, batch_list, topo):
        """the topology draws (0.0 / 1.0) of the live molecules: the host sampler's from the probabilities, or the ones
        the backend drew on the device and brought back with them"""
        sampler = self.sampling.sampler
        if sampler is None:
            draws = self.be.topo_draws
        else:
            draws = sampler.topo(t, [int(self.sampling.ids[b]) for b in batch_list], np.asarray(topo, np.float64))
        draws = np.asarray(draws, np.float64).reshape(-1)
        if draws.shape != (len(batch_list),) or not np.isin(draws, (0.0, 1.0)).all():
            raise RuntimeError("%s.decode_sampled: topology draws %r for %d molecules" % (self.NAME, draws, len(batch_list)))
        return draws

    def _beam_orders(self, t, expanding, probs, scores):
        """the order in which every expanding molecule tries its beam entries: one permutation of 0..beam-1 each.  A host
        sampler gets the probabilities, as ``torch.multinomial`` does, and the scores they are the exponentials of: a
        masked entry's probability is 0 in any format, its score is what the device ranks it by"""
        sampler = self.sampling.sampler
        if sampler is None:
            order = self.be.beam_order
        else:
            order = sampler.order(t, [int(self.sampling.ids[b]) for b in expanding], probs, scores)
        order = np.asarray(order, np.int64).reshape(len(expanding), -1)
        if not np.array_equal(np.sort(order, axis=1), np.tile(np.arange(self.beam), (len(expanding), 1))):
            raise RuntimeError("%s.decode_sampled: a drawn beam order is no permutation: %r" % (self.NAME, order))
        return order.tolist()

    def _plan(self, bid, clab, ilab, fa_node, fa_cluster, fa_used, meta, ids, cand_atoms, n_cand):
        """one beam entry: its candidates, and for several the row of the scoring launch (candidates, labels, child
        position, molecule, first score, first label, first candidate atom) -> (ismiles, candidates, attach points,
        nth_child, first score or None).  Raises what the reference's enum_attach / get_assm_score would.
        The candidates' atoms are listed only where an atom level reads them (``NA``): without one ``cand_atoms`` stays
        empty and the row's seventh column is always 0, so a backend without atom tables must not read either."""
        vocab = self.vocab
        smiles, ismiles = vocab.get_smiles(clab), vocab.get_ismiles(ilab)
        inter_cands, anchor_smiles, attach_points = self.gb.get_assm_cands(fa_cluster, fa_used, ismiles)
        if len(inter_cands) <= 1:
            return ismiles, inter_cands, attach_points, None, None
        nth = self.tree.in_degree(fa_node)
        icls = [vocab[(smiles, x)][1] for x in anchor_smiles]
        cands = inter_cands if len(attach_points) <= 2 else [(x[0], x[-1]) for x in inter_cands]
        k = len(icls)
        if k not in (1, 2) or any(_width(c) != k for c in cands):
            raise RuntimeError("enum_attach: %d attachment labels for candidates of %s atoms"
                               % (k, sorted({_width(c) for c in cands})))
        flat = () if self.NA is None else [int(a) for c in cands for a in (c if hasattr(c, "__len__") else [c])]
        if not all(0 <= int(x) < self.n_icls for x in icls) or not 0 <= nth < MAX_POS or \
                self.NA is not None and not all(0 <= a < self.NA for a in flat):
            raise IndexError("enum_attach: attachment label, child position %d or candidate atom out of range" % nth)
        meta.append((len(cands), k, nth, bid, n_cand, len(ids), len(cand_atoms)))
        ids.extend(int(x) for x in icls)
        cand_atoms.extend(flat)
        return ismiles, inter_cands, attach_points, nth, n_cand

    def _attach(self, bid, ismiles, sorted_cands, attach_points, nth_child, new_node, fa_node, results):
        """the candidates of one beam entry in order -> (the beam loop ends, success)"""
        gb, tree = self.gb, self.tree
        for cand, _ in sorted_cands:
            inter_label = list(zip(cand, attach_points))
            try:
                if not gb.try_add_mol(bid, ismiles, inter_label):
                    continue
                new_atoms, new_bonds, attached = self._add_mol(bid, ismiles, inter_label, nth_child)
            except self.CAUGHT:         # the reference's try/except: the expansion fails
                return True, False
            tree.register_cgraph(new_node, new_atoms, new_bonds, attached)
            tree.update_attached(fa_node, inter_label)
            try:
                anchors = [gb.anchor_label(ismiles, a) for a in attach_points]
            except self.CAUGHT:
                return True, False
            results[bid][-1]['Attaching Fragment'] = (ismiles, attach_points, inter_label, anchors)
            return True, True
        return False, False

    def _check_independent(self, new_mess):
        """The message kernels run every new message in its own workgroup, so none may read another of the same step.
        Holds for the decode tree: a step adds one message per molecule before its message update."""
        if len(new_mess) > 1:
            s = set(new_mess)
            if any(int(v) in s for v in self.tree.bgraph[new_mess].reshape(-1) if v):
                raise RuntimeError("%s.decode: a new message reads another message of the same step" % self.NAME)


def rnn_weights(rnn):
    """the eight weight slots of a message function, as the decode kernels take them (a GRU fills seven)"""
    if hasattr(rnn, "W_f"):
        return [rnn.W_i[0].weight, rnn.W_i[0].bias, rnn.W_o[0].weight, rnn.W_o[0].bias, rnn.W_f[0].weight,
                rnn.W_f[0].bias, rnn.W[0].weight, rnn.W[0].bias]
    return [rnn.W_z.weight, rnn.W_z.bias, rnn.W_r.weight, rnn.U_r.weight, rnn.U_r.bias, rnn.W_h.weight, rnn.W_h.bias, None]


class DeviceBackend:
    """What the two HIP backends share: the latent vectors, the vocabulary's ``owner`` table, the score heads with their
    output buffers, the uploads, the copies back and the counters of the current step (``cur``)."""

    def __init__(self, dec, src_mol_vecs, B, beam):
        F_._need_gpu(*src_mol_vecs)
        self.dec, self.B, self.beam = dec, B, beam
        self.H, self.L = H, _ = dec.hidden_size, dec.latent_size
        self.dev = dev = src_mol_vecs[0].device
        self.n_cls, self.n_icls = (int(v) for v in dec.vocab.size())
        self.src_root, self.src_tree, self.src_graph = (v.detach().float().contiguous() for v in src_mol_vecs)
        self.lib = _lib.load()
        self.lstm = hasattr(dec.hmpn.tree_encoder.rnn, "W_f")
        ld = (H + 3) // 4 * 4
        self.node_out, self.mess_out, self.hid = (torch.empty(B, ld, device=dev) for _ in range(3))
        self.topo = torch.empty(2 * B, device=dev)      # (the probabilities, then in a sampled decode their draws)
        self.sample = None                              # a sampled decode: (seed_lo, seed_hi)
        self.step = 0
        self.cls_out, self.icls_out = torch.empty(B, self.n_cls, device=dev), torch.empty(B, self.n_icls, device=dev)
        owner = getattr(dec.vocab, "owner", None)
        if owner is None:       # a PairVocab: the motif whose mask row is 0 at the attachment
            owner = torch.as_tensor(dec.vocab.mask).cpu().argmax(dim=0).numpy()
        self.owner = torch.from_numpy(np.asarray(owner, np.int32)).to(dev)
        self.new_counts()

    def new_counts(self):
        self.cur = {"launches": 0, "d2h": 0, "h2d": 0, "mess": 0, "expand": 0, "scored": 0, "wait_s": 0.0}
        return self.cur

    def _upload(self, parts):
        """one host-to-device copy of integer lists and integer or float arrays -> (buffer, offset of every part)"""
        flat = []
        for x in parts:
            if not isinstance(x, np.ndarray):
                x = np.asarray(x, np.int32)
            a = x.astype(np.float32).view(np.int32) if x.dtype.kind == "f" else x.astype(np.int32, copy=False)
            flat.append(a.reshape(-1))
        offs = np.cumsum([0] + [p.size for p in flat]).tolist()
        buf = torch.from_numpy(np.concatenate(flat + [np.zeros(1, np.int32)])).to(self.dev)
        self.cur["h2d"] += 1
        return buf, offs

    def _copy_back(self, t):
        t0 = time.perf_counter()
        out = t.cpu().numpy()
        self.cur["d2h"] += 1
        self.cur["wait_s"] += time.perf_counter() - t0
        return out

    def start_sampling(self, sampling):
        """the draws of this decode are made on the device; ``root`` takes the sample ids up"""
        self.sample = (sampling.seed_lo, sampling.seed_hi)
        self.sample_ids = sampling.ids.view(np.int32)

    def _topo_head(self, bidx, n):
        """the topology head with its sigmoid on the ``n`` read-out rows; in a sampled decode the draws are launched
        behind it, into the second half of the probabilities' buffer"""
        self._mlp(self.dec.topoNN, self.node_out, self.node_out.stride(0), bidx, n, self.topo, 1, sigmoid=True)
        if self.sample is not None:
            _lib.check(self.lib.ggpm_sample_topo(F_._p(self.topo), bidx, F_._p(self.ids_dev), n, self.step,
                                                 self.sample[0], self.sample[1], _ptr(self.topo, n), F_._stream()),
                       "sample_topo")
            self.cur["launches"] += L_DRAW

    def _read_topo(self, n):
        """the ``n`` topology probabilities copied back; in a sampled decode their draws come in the same copy
        (``topo_draws``)"""
        if self.sample is None:
            return self._copy_back(self.topo[:n])
        out = self._copy_back(self.topo[:2 * n])
        self.topo_draws = out[n:]
        return out[:n]

    def _mlp(self, seq, vecs, ld_v, bidx, M, out, ld_out, sigmoid=False):
        l1, l2 = seq[0], seq[3]
        _lib.check(self.lib.ggpm_motif_decode_mlp(
            F_._p(vecs), ld_v, bidx, F_._p(self.src_tree), self.src_tree.stride(0), M, self.H, self.L, F_._p(l1.weight),
            F_._p(l1.bias), F_._p(l2.weight), F_._p(l2.bias), l2.weight.shape[0], int(sigmoid), F_._p(self.hid),
            self.hid.stride(0), F_._p(out), ld_out, F_._stream()), "motif_decode_mlp")
        self.cur["launches"] += L_MLP

    def _heads_topk(self, vecs, ld_v, bidx, M, k, root):
        """clsNN, iclsNN and hier_topk (root: the arg-max motif and its sorted masked attachments) of M rows, launched ->
        what ``_read_topk`` copies back.  In a sampled decode the order draw is launched behind ``hier_topk`` and writes behind
        its output, so one copy brings both"""
        self._mlp(self.dec.clsNN, vecs, ld_v, bidx, M, self.cls_out, self.n_cls)
        self._mlp(self.dec.iclsNN, vecs, ld_v, bidx, M, self.icls_out, self.n_icls)
        draw = self.sample is not None and not root     # (the drawn order [M, k] behind the [M, 3k] it is drawn from)
        out = torch.empty(M * (4 if draw else 3) * k, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.ggpm_hier_topk(F_._p(self.cls_out), self.n_cls, self.n_cls, F_._p(self.icls_out), self.n_icls,
                                           self.n_icls, F_._p(self.owner), M, k, int(root), F_._p(out), F_._stream()),
                   "hier_topk")
        self.cur["launches"] += L_TOPK
        if draw:
            _lib.check(self.lib.ggpm_sample_beam_order(F_._p(out), bidx, F_._p(self.ids_dev), M, k, self.step,
                                                       self.sample[0], self.sample[1], _ptr(out, M * 3 * k),
                                                       F_._stream()), "sample_beam_order")
            self.cur["launches"] += L_DRAW
        return out, M, draw

    def _read_topk(self, launched, k):
        """``_heads_topk``'s buffer, copied back -> (scores [M, k], motifs [M, k], attachments [M, k]); the drawn order that
        came with them is ``beam_order``"""
        out, M, draw = launched
        out = self._copy_back(out)
        if draw:
            self.beam_order = out[3 * k * M:].reshape(M, k)
        out = out[:3 * k * M].reshape(M, 3 * k)
        return out[:, :k].view(np.float32), out[:, k:2 * k], out[:, 2 * k:]

    def _root_state(self):
        """the rows of the super-root messages ``root`` writes init_vecs to (LSTM: the hidden half)"""
        raise NotImplementedError

    def root(self, k0):
        """the root's heads on init_vecs -> (scores, motifs, attachments) [B, k0]"""
        dec, B, H = self.dec, self.B, self.H
        init = dec._init_vecs(self.src_root)
        parts = [np.arange(B)] + ([] if self.sample is None else [self.sample_ids])
        buf, offs = self._upload(parts)
        if self.sample is not None:
            self.ids_dev = buf[offs[1]:offs[1] + B]         # resident for the decode
        out = self._read_topk(self._heads_topk(init, F_._ld(init), _ptr(buf, offs[0]), B, k0, root=True), k0)
        self._root_state().copy_(init[:, :H])
        return out
