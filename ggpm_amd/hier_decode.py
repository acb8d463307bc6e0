"""Greedy decode of the hierarchical decoder -- reference ggpm/decoder.py:303-472 (``HierMPNDecoder.decode``) on the
library's kernels (csrc/hier_decode.hip, and the score heads and ``hier_topk`` of csrc/motif_decode.hip).

Chemistry goes through a *graph batch*, as in ``ggpm_amd.motif_decode``: the constructor ``(vocab, avocab, batch_size,
node_fdim=, edge_fdim=)``, ``add_mol`` (returning the fragment's atoms, its *directed* message ids and the parent atoms it
shares), ``get_assm_cands``, ``try_add_mol``, ``get_mol``, ``anchor_label(ismiles, atom)`` -- and ``get_tensors()`` giving
the atom-level tables ``(fnode, fmess, agraph, bgraph, _)`` of ``IncBase`` as host tensors that ``add_mol`` writes in
place.  ``ggpm_amd.synth_graph.SynthHierGraphBatch`` is a synthetic one; INTEGRATION.md (*Decoding*) shows the wrapper of
the reference's ``IncGraph``.  The reference's hierarchical decode has no try/except: whatever the graph batch, the
vocabulary or ``enum_attach`` raises there is raised here, before any launch that would read the bad value.

Host: the decode-time tree (``motif_decode.DecodeTree`` with ``cgraph``), the stacks, the graph batch, the results, and a
shadow copy of the atom tables: after each assembly the used prefix of the host tables is compared with the shadow and the
rows that differ go with the next upload (``changed_rows``) -- the graph batch is never asked which rows it touched.
Device, resident for the whole decode: the message states of the three levels (h, and c for LSTM; the atom level twice,
for its Jacobi iterations), the tree tables (shared by the tree and inter levels) with ``cgraph``, the atom tables, and the
atom read-out rows (``hgraph.node``) with the step that wrote each.  One step (launches in brackets):
  1. upload: tree and atom edits, the clusters' messages and atoms, the current nodes and their molecules.  Atom step
     [2 + diterG]: edits and reset; one launch per Jacobi iteration; read-out.  Tree step [1]: per current node the inter
     input and read-out, the tree input and read-out.  Topology head [2].  Copy the probabilities back.
  2. expand / pop on the host.  Upload: tree edits, the nodes, the new messages, the expanding molecules.  Tree step
     [5]: edits; inter inputs; inter messages; inter read-outs and tree inputs; tree messages.  clsNN [2], iclsNN [2],
     ``hier_topk`` [1].  Copy the top k back.  (No new message -- every live molecule popped its root: nothing is run.)
  3. every beam entry's candidates on the host; when some entry has several, upload them, score all in one launch [1]
     (the candidates' atom rows are those step 1 wrote), copy the scores back.
  4. assembly in the reference's order.
``LAUNCHES`` derives the counts; ``HierMPNDecoder.last_decode_stats`` holds those of every step.
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
from .motif_decode import DecodeTree, MAX_NB, MAX_SUB_NODES, _ptr, _width

ATOM_NB = 10                # IncGraph's max_nb
MAX_CLUSTER_MESS = 60       # directed messages of one cluster the kernels accept (30 atoms)
L_MLP, L_TOPK, L_ASSM = 2, 1, 1
NO_FACTORY = ("HierMPNDecoder.decode needs a graph batch (the molecule-assembly object, the reference's IncGraph): pass "
              "graph_batch_factory= (ggpm_amd.synth_graph.SynthHierGraphBatch, or the reference's IncGraph wrapped as "
              "INTEGRATION.md, section Decoding, shows), set args.graph_batch_factory for reconstruct / "
              "HierPropertyVAEOptimizer.forward, or set decoder.graph_batch_factory")


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
    factory = graph_batch_factory if graph_batch_factory is not None else getattr(dec, "graph_batch_factory", None)
    if factory is None:
        raise NotImplementedError(NO_FACTORY)
    if not greedy:
        raise NotImplementedError("HierMPNDecoder.decode: greedy=False (sampled decoding) is not part of this build; every "
                                  "caller in the reference decodes greedily")
    if dec.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in dec.modules()):
        raise NotImplementedError("HierMPNDecoder.decode runs without dropout: call model.eval() first (reconstruct.py "
                                  "does)")
    with torch.no_grad():
        run = _Decode(dec, factory, src_mol_vecs, int(max_decode_step), int(beam), backend)
        out = run.run()
    dec.last_decode_stats, dec.last_decode_tree, dec.last_decode_trace = run.stats, run.tree, run.trace
    return out


def check_limits(dec, beam, B):
    """the shapes the kernels accept; anything else raises before the first launch"""
    hmpn = dec.hmpn
    H, L = dec.hidden_size, dec.latent_size
    n_cls, n_icls = (int(v) for v in dec.vocab.size())
    if not 1 <= beam <= min(16, n_cls, n_icls):
        raise ValueError("HierMPNDecoder.decode: beam %d (1 to 16 and at most the vocabulary sizes %d / %d)"
                         % (beam, n_cls, n_icls))
    if not (1 <= H <= 1024 and 1 <= L <= 1024):
        raise ValueError("HierMPNDecoder.decode: hidden size %d / latent size %d (1 to 1024)" % (H, L))
    if dec.embed_size != H:
        raise ValueError("HierMPNDecoder.decode: embed_size must equal hidden_size (W_i reads [E_i | atom vectors] as two "
                         "embed_size halves), got %d and %d" % (dec.embed_size, H))
    if not 1 <= hmpn.atom_size + hmpn.bond_size <= 1024:
        raise ValueError("HierMPNDecoder.decode: atom message width %d (1 to 1024)" % (hmpn.atom_size + hmpn.bond_size))
    if B < 1:
        raise ValueError("HierMPNDecoder.decode: an empty batch")


def _rnn_weights(rnn):
    if hasattr(rnn, "W_f"):
        return [rnn.W_i[0].weight, rnn.W_i[0].bias, rnn.W_o[0].weight, rnn.W_o[0].bias, rnn.W_f[0].weight,
                rnn.W_f[0].bias, rnn.W[0].weight, rnn.W[0].bias]
    return [rnn.W_z.weight, rnn.W_z.bias, rnn.W_r.weight, rnn.U_r.weight, rnn.U_r.bias, rnn.W_h.weight, rnn.W_h.bias, None]


class HipBackend:
    """The device side of one decode: the resident state, the uploads, the launches and the copies back"""

    def __init__(self, dec, src_mol_vecs, B, N, E, NA, EA, beam):
        root = src_mol_vecs[0]
        F_._need_gpu(*src_mol_vecs)
        self.dec, self.B, self.beam = dec, B, beam
        self.H, self.L = H, L = dec.hidden_size, dec.latent_size
        self.dev = dev = root.device
        self.n_cls, self.n_icls = (int(v) for v in dec.vocab.size())
        self.src_root, self.src_tree, self.src_graph = (v.detach().float().contiguous() for v in src_mol_vecs)
        self.lib = _lib.load()
        hmpn = dec.hmpn
        self.lstm = hasattr(hmpn.tree_encoder.rnn, "W_f")
        self.diterT, self.diterG = hmpn.tree_encoder.rnn.depth, hmpn.graph_encoder.rnn.depth
        self.AF, self.EF = hmpn.atom_size, hmpn.atom_size + hmpn.bond_size
        ws = _rnn_weights(hmpn.graph_encoder.rnn) + _rnn_weights(hmpn.inter_encoder.rnn) + \
            _rnn_weights(hmpn.tree_encoder.rnn)
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
        ld = (H + 3) // 4 * 4
        self.node_out, self.mess_out, self.hid = (torch.empty(B, ld, **f32) for _ in range(3))
        self.topo = torch.empty(B, **f32)
        self.cls_out, self.icls_out = torch.empty(B, self.n_cls, **f32), torch.empty(B, self.n_icls, **f32)
        owner = getattr(dec.vocab, "owner", None)
        if owner is None:       # a PairVocab: the motif whose mask row is 0 at the attachment
            owner = torch.as_tensor(dec.vocab.mask).cpu().argmax(dim=0).numpy()
        self.owner = torch.from_numpy(np.asarray(owner, np.int32)).to(dev)
        self.stamp = 0
        self.spans = None           # tools/time_hier_decode.py: [(phase, start event, end event)] when a list
        self.new_counts()

    def _mark(self):
        if self.spans is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def new_counts(self):
        self.cur = {"launches": 0, "d2h": 0, "h2d": 0, "mess": 0, "expand": 0, "scored": 0, "wait_s": 0.0}
        return self.cur

    def _upload(self, parts):
        """one host-to-device copy of int32 / fp32 lists -> (buffer, offset of every list)"""
        flat = []
        for x in parts:
            a = np.asarray(x)
            a = a.astype(np.float32).view(np.int32) if a.dtype.kind == "f" else a.astype(np.int32)
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

    def _mlp(self, seq, vecs, ld_v, bidx, M, out, ld_out, sigmoid=False):
        l1, l2 = seq[0], seq[3]
        _lib.check(self.lib.ggpm_motif_decode_mlp(
            F_._p(vecs), ld_v, bidx, F_._p(self.src_tree), self.src_tree.stride(0), M, self.H, self.L, F_._p(l1.weight),
            F_._p(l1.bias), F_._p(l2.weight), F_._p(l2.bias), l2.weight.shape[0], int(sigmoid), F_._p(self.hid),
            self.hid.stride(0), F_._p(out), ld_out, F_._stream()), "motif_decode_mlp")
        self.cur["launches"] += L_MLP

    def _heads_topk(self, vecs, ld_v, bidx, M, k, root):
        self._mlp(self.dec.clsNN, vecs, ld_v, bidx, M, self.cls_out, self.n_cls)
        self._mlp(self.dec.iclsNN, vecs, ld_v, bidx, M, self.icls_out, self.n_icls)
        return self._topk(M, k, root)

    def _topk(self, M, k, root, t0=None):
        out = torch.empty(M, 3 * k, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.ggpm_hier_topk(F_._p(self.cls_out), self.n_cls, self.n_cls, F_._p(self.icls_out), self.n_icls,
                                           self.n_icls, F_._p(self.owner), M, k, int(root), F_._p(out), F_._stream()),
                   "hier_topk")
        self.cur["launches"] += L_TOPK
        if t0 is not None:
            self.spans.append(("rest", t0, self._mark()))
        out = self._copy_back(out)
        return out[:, :k].view(np.float32), out[:, k:2 * k], out[:, 2 * k:]

    def root(self, k0):
        """the root's heads on init_vecs; ``h[1:B+1] = init_vecs`` on the tree level only (LSTM: the hidden half)"""
        dec, B, H = self.dec, self.B, self.H
        if self.L == H:
            init = self.src_root
        else:
            init = F_.linear([self.src_root], [self.L], dec.W_root.weight, dec.W_root.bias)[:, :H]
        buf, offs = self._upload([np.arange(B)])
        out = self._heads_topk(init, F_._ld(init), _ptr(buf, offs[0]), B, k0, root=True)
        self.th[1:B + 1].copy_(init[:, :H])
        return out

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
        self._mlp(self.dec.topoNN, self.node_out, self.node_out.stride(0), _ptr(buf, offs[12]), n, self.topo, 1,
                  sigmoid=True)
        if t0 is not None:
            self.spans += [("atom", t0, t1), ("rest", t1, self._mark())]
        return self._copy_back(self.topo[:n])

    def phase2(self, tedits, nodes, mess, expanding, k):
        """the new messages on the inter and tree levels -> (scores, motifs, attachments) of the expanding molecules"""
        buf, offs = self._upload([tedits, nodes, mess, expanding])
        t0 = self._mark()
        self._tree_step(buf, offs[0], len(tedits), offs[1], len(nodes), offs[2], len(mess))
        self.cur["mess"] = 1
        if not len(expanding):
            if t0 is not None:
                self.spans.append(("rest", t0, self._mark()))
            return None
        self._mlp(self.dec.clsNN, self.mess_out, self.mess_out.stride(0), _ptr(buf, offs[3]), len(expanding), self.cls_out,
                  self.n_cls)
        self._mlp(self.dec.iclsNN, self.mess_out, self.mess_out.stride(0), _ptr(buf, offs[3]), len(expanding),
                  self.icls_out, self.n_icls)
        return self._topk(len(expanding), k, False, t0)

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
        if t0 is not None:
            self.spans.append(("rest", t0, self._mark()))
        return self._copy_back(score)

    def tables(self):
        """the device mirrors, read back (tests)"""
        return {k: getattr(self, k).cpu().numpy() for k in ("t_fnode", "t_fmess", "t_agraph", "t_bgraph", "t_cgraph",
                                                            "a_fnode", "a_fmess", "a_agraph", "a_bgraph")}


class _Decode:
    def __init__(self, dec, factory, src_mol_vecs, max_steps, beam, backend=None):
        self.dec, self.max_steps, self.beam = dec, max_steps, beam
        self.B = B = src_mol_vecs[0].shape[0]
        check_limits(dec, beam, B)
        self.vocab = dec.vocab
        self.n_cls, self.n_icls = (int(v) for v in dec.vocab.size())
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
        self.be = make(dec, src_mol_vecs, B, self.N, self.E, self.NA, self.EA, beam)
        self.stats, self.trace = [], []

    def _tree_edits(self):
        """the queued tree edits as quads (0 agraph / 1 bgraph / 2 fmess / 3 fnode / 4 cgraph, row, slot, value)"""
        ne, te = self.tree.take_edits()
        return np.asarray([(3, n, 0, v) for n, v in ne] + te, np.int32).reshape(-1, 4)

    def _add_mol(self, *a):
        out = self.gb.add_mol(*a)
        self.atab.note(out[0], out[1])
        return out

    # ------------------------------------------------------------------ the loop
    def run(self):
        B, vocab, gb, tree = self.B, self.vocab, self.gb, self.tree
        results = [[] for _ in range(B)]
        stack = [[] for _ in range(B)]
        # the root (decoder.py:313-350)
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
            self._step(t, batch_list, stack, results)
            for mol, r in zip(gb.get_mol(), results):
                r[-1]['partial-graph'] = mol
            self.stats.append(self.cur)
        return results, gb.get_mol()

    def _step(self, t, batch_list, stack, results):
        tree, vocab = self.tree, self.vocab
        # 1. the atom level over the current nodes' clusters, the inter and tree read-outs, the topology head (:361-370)
        nodes = [stack[b][-1] for b in batch_list]
        atoms = [int(a) for n in nodes for a in tree.cluster[n]]
        edges = [int(e) for n in nodes for e in tree.cluster_edges[n]]
        for n in nodes:
            if len(tree.cluster[n]) > MAX_SUB_NODES or len(tree.cluster_edges[n]) > MAX_CLUSTER_MESS:
                raise ValueError("HierMPNDecoder.decode: a cluster of %d atoms and %d messages (at most %d and %d)"
                                 % (len(tree.cluster[n]), len(tree.cluster_edges[n]), MAX_SUB_NODES, MAX_CLUSTER_MESS))
        if atoms and not (0 <= min(atoms) and max(atoms) < self.NA) or edges and not (0 <= min(edges) and
                                                                                      max(edges) < self.EA):
            raise IndexError("HierMPNDecoder.decode: a cluster's atom or message is outside the graph batch's tables")
        topo = self.be.phase1(self._tree_edits(), self.atab.take_edits(), edges, atoms, nodes, batch_list)
        # 2. expand or pop (:376-394), the new messages, the cluster heads of the expanding molecules
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
        if not new_mess:
            return
        self._check_messages(new_mess)
        rows = {i: q for q, (i, _) in enumerate(expand)}
        expanding = [bid for _, bid in expand]
        top = self.be.phase2(self._tree_edits(), nodes, [(e, rows.get(i, -1)) for i, e in enumerate(new_mess)],
                             expanding, self.beam)
        if not expanding:
            return
        self.cur["expand"] = 1
        scores, cls_topk, icls_topk = top
        # 3. every beam entry's candidates (get_assm_cands changes nothing); the entries with several scored in one launch.
        #    What raises here is kept with its entry and raised when the assembly reaches it, as the reference would.
        plans, meta, ids, cand_atoms = [], [], [], []
        n_cand = 0
        for i, bid in enumerate(expanding):
            fa_node = stack[bid][-2]
            fa_cluster, _, fa_used = tree.get_cluster(fa_node)
            results[bid][-1]['top-5-inter-cands'] = [(vocab.get_smiles(int(x)), vocab.get_ismiles(int(y)), float(s))
                                                     for x, y, s in zip(cls_topk[i], icls_topk[i], scores[i])]
            entries = []
            for kk in range(self.beam):
                clab, ilab = int(cls_topk[i][kk]), int(icls_topk[i][kk])
                try:
                    ent = self._plan(bid, clab, ilab, fa_node, fa_cluster, fa_used, meta, ids, cand_atoms, n_cand)
                except Exception as e:      # noqa: BLE001  (raised again in the assembly, if it gets there)
                    entries.append((clab, ilab, e))
                    break
                if ent[4] is not None:
                    n_cand += len(ent[1])
                entries.append((clab, ilab, ent))
            plans.append(entries)
        assm = None
        if meta:
            self.cur["scored"] = 1
            assm = self.be.phase3(np.asarray(meta, np.int32), ids, cand_atoms, n_cand)
            if np.isnan(assm).any():
                raise RuntimeError("HierMPNDecoder.decode: the attachment-score kernel refused a candidate table row")
        # 4. assembly (:413-454) and the forced backtrack (:456-466)
        for i, bid in enumerate(expanding):
            new_node, fa_node = stack[bid][-1], stack[bid][-2]
            success = False
            for kk, (clab, ilab, ent) in enumerate(plans[i]):
                tree.set_node_feature(new_node, clab, ilab)
                if isinstance(ent, Exception):
                    raise ent
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
                success = self._attach(bid, ismiles, sorted_cands, attach_points, nth_child, new_node, fa_node, results)
                if success:
                    break
            if not success:
                child = stack[bid].pop()
                nth = tree.in_degree(stack[bid][-1])
                tree.add_edge(child, stack[bid][-1], (child, stack[bid][-1], nth))
                child = stack[bid].pop()
                if stack[bid]:
                    nth = tree.in_degree(stack[bid][-1])
                    tree.add_edge(child, stack[bid][-1], (child, stack[bid][-1], nth))

    def _plan(self, bid, clab, ilab, fa_node, fa_cluster, fa_used, meta, ids, cand_atoms, n_cand):
        """one beam entry: its candidates, and for several the rows of the scoring launch -> (ismiles, candidates, attach
        points, nth_child, first score or None).  Raises what the reference's enum_attach would."""
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
        flat = [int(a) for c in cands for a in (c if hasattr(c, "__len__") else [c])]
        if not all(0 <= int(x) < self.n_icls for x in icls) or not 0 <= nth < MAX_POS or \
                not all(0 <= a < self.NA for a in flat):
            raise IndexError("enum_attach: attachment label, child position %d or candidate atom out of range" % nth)
        meta.append((len(cands), k, nth, bid, n_cand, len(ids), len(cand_atoms)))
        ids.extend(int(x) for x in icls)
        cand_atoms.extend(flat)
        return ismiles, inter_cands, attach_points, nth, n_cand

    def _attach(self, bid, ismiles, sorted_cands, attach_points, nth_child, new_node, fa_node, results):
        """the candidates of one beam entry in order -> success"""
        gb, tree = self.gb, self.tree
        for cand, _ in sorted_cands:
            inter_label = list(zip(cand, attach_points))
            if not gb.try_add_mol(bid, ismiles, inter_label):
                continue
            new_atoms, new_bonds, attached = self._add_mol(bid, ismiles, inter_label, nth_child)
            tree.register_cgraph(new_node, new_atoms, new_bonds, attached)
            tree.update_attached(fa_node, inter_label)
            anchors = [gb.anchor_label(ismiles, a) for a in attach_points]
            results[bid][-1]['Attaching Fragment'] = (ismiles, attach_points, inter_label, anchors)
            return True
        return False

    def _check_messages(self, new_mess):
        """The tree-level kernel runs every new message in its own workgroup, so none may read another of the same step.
        Holds for the decode tree: a step adds one message per molecule before its message update."""
        if len(new_mess) > 1:
            s = set(new_mess)
            if any(int(v) in s for v in self.tree.bgraph[new_mess].reshape(-1) if v):
                raise RuntimeError("HierMPNDecoder.decode: a new message reads another message of the same step")
