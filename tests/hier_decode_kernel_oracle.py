"""fp64 restatements of what the kernels of csrc/hier_decode.hip compute, one call at a time, and a decode backend made of
them (``OracleBackend``: the host loop of ``ggpm_amd.hier_decode.decode`` runs on it without a GPU).  CPU only (torch
fp64).

Anchors outside the code under test: every level goes through ``oracle.ref_encoder`` (``inc_mpn_forward``,
``embed_sub_tree``, ``inc_hier_forward``: the restatement of IncHierMPNEncoder that tests/test_oracle_golden.py pins to the
reference), the attachment score through ``oracle.ref_decoder.enum_attach`` and the ``get_assm_score`` expression, the
heads and the top-k selections through tests/decode_kernel_oracle.py.  The tables arrive as the device holds them: the tree's
``fnode`` [N, 2], ``fmess`` [E, 2] (source node, position), ``agraph`` / ``bgraph`` [., 12], ``cgraph`` [N, 30]; the atom
level's ``fnode`` [NA, atom_size], ``fmess`` [EA, edge_fdim] (fp32), ``agraph`` / ``bgraph`` [EA, 10].

Parameters arrive under the decoder's ``state_dict`` names (``hmpn.graph_encoder.rnn.W_z.weight``, ``matchNN.0.weight``).
"""
import numpy as np
import torch

import decode_kernel_oracle as O
from oracle import ref_decoder as RD
from oracle import ref_encoder as R

MAX_POS = 20
f64 = O.f64


def _lt(v):
    return torch.as_tensor(np.asarray(v, dtype=np.int64)).reshape(-1) if np.asarray(v).ndim <= 1 else \
        torch.as_tensor(np.asarray(v, dtype=np.int64))


def _d(v):
    return torch.as_tensor(np.asarray(v)).double()


def hmpn(p):
    return RD._sub(p, "hmpn.")


def _state(rnn, h, c):
    return _d(h) if rnn == "GRU" else (_d(h), _d(c))


# ---------------------------------------------------------------------------------------------- atom level
def atom_step(p, rnn, depth, h, c, fnode, fmess, agraph, bgraph, edges, atoms):
    """IncMPNEncoder.forward of the atom level on (atoms, edges): reset, ``depth`` Jacobi iterations, the read-out ->
    (h, c after it [EA, H] (c None for GRU), read-out rows [len(atoms), H])"""
    sub = (_lt(atoms), _lt(edges))
    tens = R._sub_tensor([_d(fnode), _d(fmess), _lt(agraph), _lt(bgraph)], sub)
    node, st = R.inc_mpn_forward(hmpn(p), "graph_encoder.", rnn, depth, tens, _state(rnn, h, c), len(fnode), sub)
    hh, cc = (st, None) if rnn == "GRU" else st
    return hh, cc, node.index_select(0, sub[0])


def atom_step_gauss_seidel(p, rnn, depth, h, c, fmess, bgraph, edges):
    """what a kernel that updated the rows in place, one after the other, would give (the bug the Jacobi test excludes)
    -> h after it"""
    ph = hmpn(p)
    h = _d(h).clone()
    c = None if rnn == "GRU" else _d(c).clone()
    edges = [int(e) for e in edges]
    h[edges] = 0
    if c is not None:
        c[edges] = 0
    fm, bg = _d(fmess), _lt(bgraph)
    for _ in range(depth):
        for e in edges:
            x, nb = fm[e:e + 1], bg[e:e + 1]
            if rnn == "GRU":
                h[e] = R.gru_cell(ph, "graph_encoder.rnn.", x, R.gather_rows(h, nb))[0]
            else:
                hn, cn = R.lstm_cell(ph, "graph_encoder.rnn.", x, R.gather_rows(h, nb), R.gather_rows(c, nb))
                h[e], c[e] = hn[0], cn[0]
    return h


# ---------------------------------------------------------------------------------------------- inter and tree levels
def tree_tensors(fnode, fmess, agraph, bgraph, cgraph):
    fm = _lt(fmess)
    fm3 = torch.stack([fm[:, 0], torch.zeros_like(fm[:, 0]), fm[:, 1]], dim=1)
    return [_lt(fnode), fm3, _lt(agraph), _lt(bgraph), _lt(cgraph), None]


def tree_step(p, rnn, depth, tabs, anode, ih, ic, th, tc, nodes, mess):
    """the inter level, then the tree level, on (nodes, mess) with the atom read-outs ``anode`` [NA, H] (zero rows where
    the step's atom level wrote none) -> dict: the two levels' node inputs and read-outs of ``nodes`` and their states"""
    ph = hmpn(p)
    tt = tree_tensors(*tabs)
    sub = (_lt(nodes), _lt(mess))
    n_tree = len(tabs[0])
    s = R.embed_sub_tree(ph, tt, _d(anode), sub, True)
    inode, ist = R.inc_mpn_forward(ph, "inter_encoder.", rnn, depth, s, _state(rnn, ih, ic), n_tree, sub)
    s2 = R.embed_sub_tree(ph, tt, inode, sub, False)
    tnode, tst = R.inc_mpn_forward(ph, "tree_encoder.", rnn, depth, s2, _state(rnn, th, tc), n_tree, sub)
    hid = (lambda st: st if rnn == "GRU" else st[0])
    cel = (lambda st: None if rnn == "GRU" else st[1])
    return {"xi": s[0], "xc": s2[0], "inode": inode.index_select(0, sub[0]), "tnode": tnode.index_select(0, sub[0]),
            "ih": hid(ist), "ic": cel(ist), "th": hid(tst), "tc": cel(tst)}


# ---------------------------------------------------------------------------------------------- attachment score
def assm_score(p, anode, cands, icls, nth, z_row):
    """enum_attach + get_assm_score of one prediction: ``cands`` [n, k] atoms -> [n] scores"""
    v = RD.enum_attach(p, _d(anode), _lt(np.asarray(cands).reshape(len(cands), -1)), list(icls), int(nth))
    return (R._affine(p, "W_assm", v) * _d(z_row).unsqueeze(0)).sum(dim=-1)


# ---------------------------------------------------------------------------------------------- a decode backend
class OracleBackend:
    """``ggpm_amd.hier_decode.HipBackend``'s interface in fp64 on the CPU.  It keeps its own mirrors of the tables and
    brings them up to date from the edits alone, as the device does."""

    def __init__(self, dec, src_mol_vecs, B, N, E, NA, EA, beam):
        self.dec, self.B = dec, B
        self.p = f64({k: v.detach().cpu().numpy() for k, v in dec.state_dict().items()})
        self.H, self.L = dec.hidden_size, dec.latent_size
        self.rnn = "LSTM" if hasattr(dec.hmpn.tree_encoder.rnn, "W_f") else "GRU"
        self.dT, self.dG = dec.hmpn.tree_encoder.rnn.depth, dec.hmpn.graph_encoder.rnn.depth
        self.src = [_d(v.detach().cpu().numpy()) for v in src_mol_vecs]
        AF, EF, H = dec.hmpn.atom_size, dec.hmpn.atom_size + dec.hmpn.bond_size, self.H
        self.tt = [np.zeros((N, 2), np.int64), np.zeros((E, 2), np.int64), np.zeros((N, 12), np.int64),
                   np.zeros((E, 12), np.int64), np.zeros((N, 30), np.int64)]
        self.at = [np.zeros((NA, AF)), np.zeros((EA, EF)), np.zeros((EA, 10), np.int64), np.zeros((EA, 10), np.int64)]
        z = lambda n: torch.zeros(n, H, dtype=torch.float64)        # noqa: E731
        self.gh, self.gc, self.ih, self.ic, self.th, self.tc = z(EA), z(EA), z(E), z(E), z(E), z(E)
        self.anode = z(NA)
        owner = getattr(dec.vocab, "owner", None)
        self.owner = np.asarray(owner if owner is not None else torch.as_tensor(dec.vocab.mask).argmax(dim=0).numpy())
        self.new_counts()

    def new_counts(self):
        self.cur = {"launches": 0, "d2h": 0, "h2d": 0, "mess": 0, "expand": 0, "scored": 0, "wait_s": 0.0}
        return self.cur

    def _heads(self, vecs, bidx, k, root):
        return O.heads_topk(self.p, vecs, self.src[1][_lt(bidx)], self.owner, k, root)

    def root(self, k0):
        init = self.src[0] if self.L == self.H else R._affine(self.p, "W_root", self.src[0])
        self.th[1:self.B + 1] = init
        return self._heads(init, np.arange(self.B), k0, True)

    def _tree_edits(self, tedits):
        for tab, row, slot, v in np.asarray(tedits).reshape(-1, 4):
            t = {0: self.tt[2], 1: self.tt[3], 2: self.tt[1], 3: self.tt[0], 4: self.tt[4]}[int(tab)]
            t[row, slot] = v

    def phase1(self, tedits, aedits, edges, atoms, nodes, bidx):
        self._tree_edits(tedits)
        for t, (rows, vals) in zip(self.at, aedits):
            t[rows] = vals
        self.gh, gc, rows = atom_step(self.p, self.rnn, self.dG, self.gh, self.gc, *self.at, edges, atoms)
        self.gc = self.gc if gc is None else gc
        self.anode = torch.zeros_like(self.anode)       # hgraph.node is rebuilt from zeros
        self.anode[_lt(atoms)] = rows
        out = tree_step(self.p, self.rnn, self.dT, self.tt, self.anode, self.ih, self.ic, self.th, self.tc, nodes, [])
        w = [self.p["topoNN" + n] for n in (".0.weight", ".0.bias", ".3.weight", ".3.bias")]
        return O.mlp(out["tnode"], self.src[1][_lt(bidx)], *w, sigmoid=True)[1].reshape(-1).numpy()

    def phase2(self, tedits, nodes, mess, expanding, k):
        if not len(mess):
            return None
        self._tree_edits(tedits)
        mess = np.asarray(mess).reshape(-1, 2)
        out = tree_step(self.p, self.rnn, self.dT, self.tt, self.anode, self.ih, self.ic, self.th, self.tc, nodes,
                        mess[:, 0])
        self.ih, self.th = out["ih"], out["th"]
        if self.rnn == "LSTM":
            self.ic, self.tc = out["ic"], out["tc"]
        if not len(expanding):
            return None
        rows = mess[mess[:, 1] >= 0]
        vecs = torch.zeros(len(expanding), self.H, dtype=torch.float64)
        vecs[_lt(rows[:, 1])] = self.th[_lt(rows[:, 0])]
        return self._heads(vecs, expanding, k, False)

    def phase3(self, meta, ids, atoms, n_cand):
        out = np.zeros(n_cand)
        for n, k, nth, b, coff, roff, aoff in np.asarray(meta).reshape(-1, 7):
            cands = np.asarray(atoms[aoff:aoff + n * k]).reshape(n, k)
            out[coff:coff + n] = assm_score(self.p, self.anode, cands, ids[roff:roff + k], nth, self.src[2][b]).numpy()
        return out
