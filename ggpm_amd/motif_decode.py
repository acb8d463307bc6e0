"""Greedy decode of the tree-only decoder -- reference ggpm/decoder.py:901-1095 (``MotifDecoder.decode``): what
``ggpm_amd.greedy_decode``'s loop needs to be that decoder's, and its device backend on the library's kernels
(csrc/motif_decode.hip).

The graph batch's constructor is ``(vocab, avocab, batch_size, max_nodes=, max_edges=, node_fdim=, edge_fdim=)``;
``ggpm_amd.synth_graph.SynthGraphBatch`` is a synthetic one.  An exception the graph batch (or the vocabulary lookup of an
anchor) raises in the candidate loop ends that molecule's expansion, as the reference's try/except (decoder.py:1037)
does; nothing else is caught.

Device, resident for the whole decode: the message states (h, and c for LSTM) and the tree's tables (motif ids, fmess,
agraph, bgraph).  Every phase is one upload, its launches and one copy back: the tree step with the read-outs and the
topology head [2 + 2]; the tree step with the new messages [2], then for the expanding molecules the cluster heads and
``hier_topk`` [2 + 2 + 1]; the attachment scores [1].  At most 12 launches per step; a sampled decode
(``decode_sampled``) adds the topology draw [1] behind the sigmoid head and the order draw [1] behind ``hier_topk``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import functional as F_
from . import greedy_decode as G
from . import _lib
from .decoder_heads import MAX_POS
from .greedy_decode import DecodeTree, L_ASSM, MAX_NB, _ptr

L_TREE = 2                                      # launches of the tree step
NO_FACTORY = G.no_factory("MotifDecoder", "SynthGraphBatch", "PropertyVAEOptimizer")


def decode(dec, mols, src_mol_vecs, greedy=True, max_decode_step=100, beam=5, graph_batch_factory=None, backend=None):
    """``MotifDecoder.decode`` -> (results, graph_batch.get_mol())"""
    return G.decode(_Decode, dec, src_mol_vecs, greedy, max_decode_step, beam, graph_batch_factory, backend)


def decode_sampled(dec, mols, src_mol_vecs, seed=None, sample_ids=None, max_decode_step=100, beam=5,
                   graph_batch_factory=None, backend=None, sampler=None):
    """``MotifDecoder.decode_sampled``: the reference's ``decode(greedy=False)`` on a seeded stream ->
    (results, graph_batch.get_mol())"""
    return G.decode_sampled(_Decode, dec, src_mol_vecs, seed, sample_ids, max_decode_step, beam, graph_batch_factory,
                            backend, sampler)


class HipBackend(G.DeviceBackend):
    """The device side of one decode: the resident tree, the uploads, the launches and the copies back.  It has no atom
    level: ``phase1`` ignores the atom inputs, and ``phase3`` gets no candidate atoms."""

    def __init__(self, dec, src_mol_vecs, B, N, E, beam):
        super().__init__(dec, src_mol_vecs, B, beam)
        hmpn, H, dev = dec.hmpn, self.H, self.dev
        te = hmpn.tree_encoder
        ws = [hmpn.E_c[0].weight, te.W_o[0].weight, te.W_o[0].bias] + [w for w in G.rnn_weights(te.rnn) if w is not None]
        self.params = [p.detach().contiguous() for p in ws]
        self.param_ptrs = (ctypes.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        self.depth = te.rnn.depth
        self.N, self.E = N, E
        i32 = dict(dtype=torch.int32, device=dev)
        self.fnode, self.fmess = torch.zeros(N, **i32), torch.zeros(E, 2, **i32)
        self.agraph, self.bgraph = torch.zeros(N, MAX_NB, **i32), torch.zeros(E, MAX_NB, **i32)
        self.h = torch.zeros(E, H, device=dev)
        self.c = torch.zeros(E, H, device=dev) if self.lstm else None

    def _root_state(self):
        return self.h[1:self.B + 1]

    def _upload_edits(self, tedits, lists):
        """One host-to-device copy: the tree edits as the tree step reads them -- the motif of a node (table 3 of a tree
        without cgraph) as a pair, the others as quads -- then ``lists`` -> (buffer, node edits, table edits, offset of
        every list)"""
        n = int(np.count_nonzero(tedits[:, 0] == 3))        # (they come first)
        ne, te = tedits[:n, 1::2], tedits[n:]
        buf, offs = self._upload([ne, te] + lists)
        return buf, len(ne), len(te), offs[2:]

    def _tree_step(self, buf, n_ne, n_te, nodes_off=0, n_read=0, mess_off=0, n_mess=0):
        _lib.check(self.lib.ggpm_motif_decode_tree_step(
            int(self.lstm), self.H, MAX_POS, self.depth, self.param_ptrs, F_._p(self.fnode), F_._p(self.fmess),
            F_._p(self.agraph), F_._p(self.bgraph), self.N, self.E, F_._p(self.h), F_._p(self.c), _ptr(buf), n_ne, n_te,
            _ptr(buf, nodes_off), n_read, F_._p(self.node_out), self.node_out.stride(0), _ptr(buf, mess_off), n_mess,
            F_._p(self.mess_out), self.mess_out.stride(0), F_._stream()), "motif_decode_tree_step")
        self.cur["launches"] += L_TREE

    def phase1(self, tedits, aedits, edges, atoms, nodes, bidx):
        """-> the topology probabilities of ``nodes``"""
        n = len(nodes)
        buf, n_ne, n_te, offs = self._upload_edits(tedits, [nodes, bidx])
        self._tree_step(buf, n_ne, n_te, nodes_off=offs[0], n_read=n)
        self._topo_head(_ptr(buf, offs[1]), n)
        return self._read_topo(n)

    def phase2(self, tedits, nodes, mess, expanding, k):
        """the new messages (none: the upload and the tree step are still issued, for the edits) -> (scores, motifs,
        attachments) of the expanding molecules"""
        buf, n_ne, n_te, offs = self._upload_edits(tedits, [mess, expanding])
        self._tree_step(buf, n_ne, n_te, mess_off=offs[0], n_mess=len(mess))
        if not len(expanding):
            return None
        out = self._heads_topk(self.mess_out, self.mess_out.stride(0), _ptr(buf, offs[1]), len(expanding), k, root=False)
        return self._read_topk(out, k)

    def phase3(self, meta, ids, atoms, n_cand):
        buf, offs = self._upload([meta[:, :6], ids])        # (the seventh column locates the candidates' atoms)
        score = torch.empty(n_cand, device=self.dev)
        l1, wa = self.dec.matchNN[0], self.dec.W_assm
        _lib.check(self.lib.ggpm_motif_decode_assm_score(
            F_._p(self.dec.E_assm[0].weight), self.n_icls, self.H, self.L, _ptr(buf, offs[0]), _ptr(buf, offs[1]),
            len(meta),
            F_._p(l1.weight), l1.weight.stride(0), F_._p(l1.bias), F_._p(wa.weight), F_._p(wa.bias),
            F_._p(self.src_graph), self.src_graph.stride(0), F_._p(score), F_._stream()), "motif_decode_assm_score")
        self.cur["launches"] += L_ASSM
        return self._copy_back(score)


class _Decode(G.GreedyDecode):
    NAME, NO_FACTORY = "MotifDecoder", NO_FACTORY
    CAUGHT = (Exception,)
    ROOT_ATTACHMENT_POINTS = True

    def _setup(self, factory, src_mol_vecs, backend):
        dec, B = self.dec, self.B
        G.check_beam(self.NAME, dec, self.beam)
        hmpn = dec.hmpn
        self.gb = factory(dec.vocab, dec.avocab, B, max_nodes=400, max_edges=500, node_fdim=hmpn.atom_size,
                          edge_fdim=hmpn.atom_size + hmpn.bond_size)
        N = 2 + B + B * self.max_steps          # a step adds at most one node per molecule
        E = 1 + B + 3 * B * self.max_steps      # ... and at most three messages (expand, then a forced backtrack)
        self.tree = DecodeTree(N, E)
        self.be = (backend if backend is not None else HipBackend)(dec, src_mol_vecs, B, N, E, self.beam)
