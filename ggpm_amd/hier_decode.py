"""Greedy decode of the hierarchical decoder -- reference ggpm/decoder.py:303-472 (``HierMPNDecoder.decode``): what
``ggpm_amd.greedy_decode``'s loop needs to be that decoder's, and its device backend on the library's kernels
(csrc/hier_decode.hip, and the score heads and ``hier_topk`` of csrc/motif_decode.hip).

The graph batch's constructor is ``(vocab, avocab, batch_size, node_fdim=, edge_fdim=)``, and it has ``get_tensors()``
giving the atom-level tables ``(fnode, fmess, agraph, bgraph, _)`` of ``IncBase`` as host tensors that ``add_mol`` writes in
place.  ``ggpm_amd.synth_graph.SynthHierGraphBatch`` is a synthetic one.  The reference's hierarchical decode has no
try/except: whatever the graph batch, the vocabulary or ``enum_attach`` raises there is raised here, before any launch
that would read the bad value.

Host, besides the loop's: a shadow copy of the atom tables.  After each assembly the used prefix of the host tables is
compared with the shadow and the rows that differ go with the next upload (``changed_rows``) -- the graph batch is never
asked which rows it touched.
Device, resident for the whole decode: the message states of the three levels (h, and c for LSTM; the atom level twice,
for its Jacobi iterations), the tree tables (shared by the tree and inter levels) with ``cgraph``, the atom tables, and the
atom read-out rows (``hgraph.node``) with the step that wrote each.  Every phase is one upload, its launches (in brackets)
and one copy back:
  1. tree and atom edits, the clusters' messages and atoms, the current nodes and their molecules.  Atom step
     [2 + diterG]: edits and reset; one launch per Jacobi iteration; read-out.  Tree step [1]: per current node the inter
     input and read-out, the tree input and read-out.  Topology head [2].
  2. tree edits, the nodes, the new messages, the expanding molecules.  Tree step [5]: edits; inter inputs; inter
     messages; inter read-outs and tree inputs; tree messages.  clsNN [2], iclsNN [2], ``hier_topk`` [1].  (No new message
     -- every live molecule popped its root: nothing is run.)
  3. the candidates' rows, labels and atoms; all scored in one launch [1] (the atom rows are those phase 1 wrote).
``LAUNCHES`` derives the counts.  A sampled decode (``decode_sampled``) adds the topology draw [1] to phase 1 and the order
draw [1] to phase 2, into the buffers those phases copy back anyway.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import functional as F_
from . import greedy_decode as G
from .decoder_heads import MAX_POS
from .greedy_decode import DecodeTree, L_ASSM, L_MLP, L_TOPK, MAX_NB, MAX_SUB_NODES, _ptr

ATOM_NB = 10                # IncGraph's max_nb
MAX_CLUSTER_MESS = 60       # directed messages of one cluster the kernels accept (30 atoms)
NO_FACTORY = G.no_factory("HierMPNDecoder", "SynthHierGraphBatch", "HierPropertyVAEOptimizer")


def LAUNCHES(diterG, diterT=1):
    """launches of a step's three device phases -> (topology, expansion, scoring); the tree levels iterate inside their
    launch, so ``diterT`` does not count"""
    return (2 + diterG) + 1 + L_MLP, 5 + 2 * L_MLP + L_TOPK, L_ASSM


def changed_rows(host, shadow, n):
    """rows below ``n`` in which ``host`` differs from ``shadow`` (sorted); ``shadow`` is brought up to date"""
    if n <= 0:
        return np.zeros(0, np.int64)
    rows = np.nonzero((host[:n] != shadow[:n]).any(axis=1))[0]
    shadow[rows] = host[rows]
    return rows


class AtomTables:
    """The graph batch's four atom tables (host, written in place by ``add_mol``) with their shadow copies"""

    NAMES = ("fnode", "fmess", "agraph", "bgraph")

    def __init__(self, tensors):
        self.host = [np.asarray(t.numpy() if isinstance(t, torch.Tensor) else t) for t in tensors[:4]]
        for name, t, kind in zip(self.NAMES, self.host, "ffii"):
            if t.ndim != 2 or t.dtype.kind != kind:
                raise TypeError("graph batch: get_tensors() %s must be a host %s matrix, got %s %s"
                                % (name, "float" if kind == "f" else "integer", t.dtype, t.shape))
        self.shadow = [np.zeros_like(t) for t in self.host]
        self.n_atoms = self.n_mess = 1          # used prefixes (row 0 is the pad)

    def note(self, atoms, bonds):
        """``add_mol`` returned these atoms and directed messages: the used prefixes grow to hold them"""
        self.n_atoms = max([self.n_atoms] + [int(a) + 1 for a in atoms])
        self.n_mess = max([self.n_mess] + [int(e) + 1 for e in bonds])

    def take_edits(self):
        """-> [(rows, their values)] per table, the rows that changed since the last call"""
        out = []
        for host, shadow, n in zip(self.host, self.shadow, (self.n_atoms, self.n_mess, self.n_atoms, self.n_mess)):
            rows = changed_rows(host, shadow, min(n, len(host)))
            out.append((rows, host[rows]))
        return out


def decode(dec, mols, src_mol_vecs, greedy=True, max_decode_step=100, beam=5, graph_batch_factory=None, backend=None):
    """``HierMPNDecoder.decode`` -> (results, graph_batch.get_mol())"""
    return G.decode(_Decode, dec, src_mol_vecs, greedy, max_decode_step, beam, graph_batch_factory, backend)


def decode_sampled(dec, mols, src_mol_vecs, seed=None, sample_ids=None, max_decode_step=100, beam=5,
                   graph_batch_factory=None, backend=None, sampler=None):
    """``HierMPNDecoder.decode_sampled``: the reference's ``decode(greedy=False)`` on a seeded stream ->
    (results, graph_batch.get_mol())"""
    return G.decode_sampled(_Decode, dec, src_mol_vecs, seed, sample_ids, max_decode_step, beam, graph_batch_factory,
                            backend, sampler)


def check_limits(dec, beam, B):
    """the shapes the kernels accept; anything else raises before the first launch"""
    hmpn = dec.hmpn
    H, L = dec.hidden_size, dec.latent_size
    G.check_beam("HierMPNDecoder", dec, beam)
    if not (1 <= H <= 1024 and 1 <= L <= 1024):
        raise ValueError("HierMPNDecoder.decode: hidden size %d / latent size %d (1 to 1024)" % (H, L))
    if dec.embed_size != H:
        raise ValueError("HierMPNDecoder.decode: embed_size must equal hidden_size (W_i reads [E_i | atom vectors] as two "
                         "embed_size halves), got %d and %d" % (dec.embed_size, H))
    if not 1 <= hmpn.atom_size + hmpn.bond_size <= 1024:
        raise ValueError("HierMPNDecoder.decode: atom message width %d (1 to 1024)" % (hmpn.atom_size + hmpn.bond_size))
    if B < 1:
        raise ValueError("HierMPNDecoder.decode: an empty batch")


class HipBackend(G.DeviceBackend):
    """The device side of one decode: the resident state, the uploads, the launches and the copies back"""

    def __init__(self, dec, src_mol_vecs, B, N, E, NA, EA, beam):
        super().__init__(dec, src_mol_vecs, B, beam)
        H, dev, hmpn = self.H, self.dev, dec.hmpn
        self.diterT, self.diterG = hmpn.tree_encoder.rnn.depth, hmpn.graph_encoder.rnn.depth
        self.AF, self.EF = hmpn.atom_size, hmpn.atom_size + hmpn.bond_size
        ws = G.rnn_weights(hmpn.graph_encoder.rnn) + G.rnn_weights(hmpn.inter_encoder.rnn) + \
            G.rnn_weights(hmpn.tree_encoder.rnn)
        ws += [hmpn.graph_encoder.W_o[0].weight, hmpn.graph_encoder.W_o[0].bias, hmpn.inter_encoder.W_o[0].weight,
               hmpn.inter_encoder.W_o[0].bias, hmpn.tree_encoder.W_o[0].weight, hmpn.tree_encoder.W_o[0].bias,
               hmpn.E_i[0].weight, hmpn.E_c[0].weight, hmpn.W_i[0].weight, hmpn.W_i[0].bias, hmpn.W_c[0].weight,
               hmpn.W_c[0].bias]
        self.params = [None if p is None else p.detach().float().contiguous() for p in ws]
        self.param_ptrs = (ctypes.c_void_p * len(self.params))(*[None if p is None else p.data_ptr()
                                                                 for p in self.params])
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.N, self.E, self.NA, self.EA = N, E, NA, EA
        self.t_fnode, self.t_fmess = torch.zeros(N, 2, **i32), torch.zeros(E, 2, **i32)
        self.t_agraph, self.t_bgraph = torch.zeros(N, MAX_NB, **i32), torch.zeros(E, MAX_NB, **i32)
        self.t_cgraph = torch.zeros(N, MAX_SUB_NODES, **i32)
        self.a_fnode, self.a_fmess = torch.zeros(NA, self.AF, **f32), torch.zeros(EA, self.EF, **f32)
        self.a_agraph, self.a_bgraph = torch.zeros(EA, ATOM_NB, **i32), torch.zeros(EA, ATOM_NB, **i32)
        self.gh = [torch.zeros(EA, H, **f32) for _ in range(2)]
        self.gc = [torch.zeros(EA, H, **f32) for _ in range(2)] if self.lstm else [None, None]
        self.anode, self.astamp = torch.zeros(NA, H, **f32), torch.zeros(NA, **i32)
        self.ih, self.th = torch.zeros(E, H, **f32), torch.zeros(E, H, **f32)
        self.ic, self.tc = (torch.zeros(E, H, **f32), torch.zeros(E, H, **f32)) if self.lstm else (None, None)
        self.xi, self.xc = torch.zeros(B, H, **f32), torch.zeros(B, H, **f32)
        state = [self.t_fnode, self.t_fmess, self.t_agraph, self.t_bgraph, self.t_cgraph, self.a_fnode, self.a_fmess,
                 self.a_agraph, self.a_bgraph, self.gh[0], self.gh[1], self.gc[0], self.gc[1], self.anode, self.astamp,
                 self.ih, self.ic, self.th, self.tc, self.xi, self.xc]
        self.state_ptrs = (ctypes.c_void_p * len(state))(*[None if t is None else t.data_ptr() for t in state])
        dims = [int(self.lstm), H, MAX_POS, N, E, NA, EA, self.AF, self.EF, self.diterT, self.diterG, self.n_cls,
                self.n_icls, B]
        self.dims = (ctypes.c_int * len(dims))(*dims)
        self.stamp = 0
        self.spans = None           # tools/time_hier_decode.py: [(phase, start event, end event)] when a list

    def _mark(self):
        if self.spans is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _launched(self, t0):
        if t0 is not None:
            self.spans.append(("rest", t0, self._mark()))

    def _root_state(self):
        return self.th[1:self.B + 1]        # (the tree level only)

    def _tree_step(self, buf, off_edits, n_edits, off_nodes, n_nodes, off_mess, n_mess):
        _lib.check(self.lib.ggpm_hier_decode_tree_step(
            self.dims, self.state_ptrs, self.param_ptrs, _ptr(buf, off_edits), n_edits, _ptr(buf, off_nodes), n_nodes,
            _ptr(buf, off_mess), n_mess, self.stamp, F_._p(self.node_out), self.node_out.stride(0), F_._p(self.mess_out),
            self.mess_out.stride(0), F_._stream()), "hier_decode_tree_step")
        self.cur["launches"] += 5 if n_mess else 1

    def phase1(self, tedits, aedits, edges, atoms, nodes, bidx):
        """-> the topology probabilities of ``nodes``"""
        parts = [tedits]
        for rows, vals in aedits:
            parts += [rows, vals]
        buf, offs = self._upload(parts + [edges, atoms, nodes, bidx])
        counts = [len(tedits)] + [len(r) for r, _ in aedits] + [len(edges), len(atoms)]
        self.stamp += 1
        t0 = self._mark()
        _lib.check(self.lib.ggpm_hier_decode_atom_step(
            self.dims, self.state_ptrs, self.param_ptrs, _ptr(buf), (ctypes.c_int * 12)(*offs[:12]),
            (ctypes.c_int * 7)(*counts), self.stamp, F_._stream()), "hier_decode_atom_step")
        self.cur["launches"] += 2 + self.diterG
        t1 = self._mark()
        n = len(nodes)
        self._tree_step(buf, 0, 0, offs[11], n, 0, 0)
        self._topo_head(_ptr(buf, offs[12]), n)
        if t0 is not None:
            self.spans += [("atom", t0, t1), ("rest", t1, self._mark())]
        return self._read_topo(n)

    def phase2(self, tedits, nodes, mess, expanding, k):
        """the new messages on the inter and tree levels (none: nothing is run) -> (scores, motifs, attachments) of the
        expanding molecules"""
        if not len(mess):
            return None
        buf, offs = self._upload([tedits, nodes, mess, expanding])
        t0 = self._mark()
        self._tree_step(buf, offs[0], len(tedits), offs[1], len(nodes), offs[2], len(mess))
        if not len(expanding):
            self._launched(t0)
            return None
        out = self._heads_topk(self.mess_out, self.mess_out.stride(0), _ptr(buf, offs[3]), len(expanding), k, root=False)
        self._launched(t0)
        return self._read_topk(out, k)

    def phase3(self, meta, ids, atoms, n_cand):
        buf, offs = self._upload([meta, ids, atoms])
        score = torch.empty(n_cand, device=self.dev)
        l1, wa = self.dec.matchNN[0], self.dec.W_assm
        t0 = self._mark()
        _lib.check(self.lib.ggpm_hier_decode_assm_score(
            self.dims, self.state_ptrs, F_._p(self.dec.E_assm[0].weight), _ptr(buf, offs[0]), _ptr(buf, offs[1]),
            _ptr(buf, offs[2]), len(meta), n_cand, len(ids), len(np.asarray(atoms).reshape(-1)), F_._p(l1.weight), l1.weight.stride(0), F_._p(l1.bias),
            F_._p(wa.weight), F_._p(wa.bias), self.L, F_._p(self.src_graph), self.src_graph.stride(0), self.stamp,
            F_._p(score), F_._stream()), "hier_decode_assm_score")
        self.cur["launches"] += L_ASSM
        self._launched(t0)
        return self._copy_back(score)

    def tables(self):
        """the device mirrors, read back (tests)"""
        return {k: getattr(self, k).cpu().numpy() for k in ("t_fnode", "t_fmess", "t_agraph", "t_bgraph", "t_cgraph",
                                                            "a_fnode", "a_fmess", "a_agraph", "a_bgraph")}


class _Decode(G.GreedyDecode):
    NAME, NO_FACTORY = "HierMPNDecoder", NO_FACTORY

    def _setup(self, factory, src_mol_vecs, backend):
        dec, B = self.dec, self.B
        check_limits(dec, self.beam, B)
        hmpn = dec.hmpn
        self.gb = factory(dec.vocab, dec.avocab, B, node_fdim=hmpn.atom_size, edge_fdim=hmpn.atom_size + hmpn.bond_size)
        self.atab = AtomTables(self.gb.get_tensors())
        fn, fm, ag, bg = self.atab.host
        if fn.shape[1] != hmpn.atom_size or fm.shape[1] != hmpn.atom_size + hmpn.bond_size or \
                ag.shape[1] != ATOM_NB or bg.shape[1] != ATOM_NB:
            raise ValueError("graph batch: atom tables of widths %d / %d / %d / %d, the decoder reads %d / %d / %d / %d"
                             % (fn.shape[1], fm.shape[1], ag.shape[1], bg.shape[1], hmpn.atom_size,
                                hmpn.atom_size + hmpn.bond_size, ATOM_NB, ATOM_NB))
        self.N, self.E = 100 * B, 200 * B           # IncTree's defaults (decoder.py:308): a fuller tree raises there too
        self.NA, self.EA = len(fn), min(len(fm), len(bg))
        self.tree = DecodeTree(self.N, self.E, MAX_NB, cgraph=True)
        make = backend if backend is not None else HipBackend
        self.be = make(dec, src_mol_vecs, B, self.N, self.E, self.NA, self.EA, self.beam)

    def _atom_inputs(self, nodes):
        tree = self.tree
        atoms = [int(a) for n in nodes for a in tree.cluster[n]]
        edges = [int(e) for n in nodes for e in tree.cluster_edges[n]]
        for n in nodes:
            if len(tree.cluster[n]) > MAX_SUB_NODES or len(tree.cluster_edges[n]) > MAX_CLUSTER_MESS:
                raise ValueError("HierMPNDecoder.decode: a cluster of %d atoms and %d messages (at most %d and %d)"
                                 % (len(tree.cluster[n]), len(tree.cluster_edges[n]), MAX_SUB_NODES, MAX_CLUSTER_MESS))
        if atoms and not (0 <= min(atoms) and max(atoms) < self.NA) or edges and not (0 <= min(edges) and
                                                                                      max(edges) < self.EA):
            raise IndexError("HierMPNDecoder.decode: a cluster's atom or message is outside the graph batch's tables")
        return self.atab.take_edits(), edges, atoms
