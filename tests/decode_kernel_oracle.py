"""fp64 restatements of what the greedy-decode kernels (csrc/motif_decode.hip) compute, one call at a time, and the
seeded inputs the kernel tests share with tests/golden/make_golden_topk.py, and a decode backend made of them
(``OracleBackend``: ``ggpm_amd.motif_decode``'s host loop runs on it without a GPU).  CPU only (numpy / torch fp64).

Anchors outside the code under test:
  * the message update and the read-out go through ``oracle.ref_encoder`` (``gru_sparse_forward`` / ``lstm_sparse_forward``,
    the ``W_o`` expression of ``mpn_forward``), the attachment score through ``oracle.ref_decoder.enum_attach`` and the
    ``get_assm_score`` expression of ``ref_encoder.score_heads`` -- all pinned to the reference by
    tests/test_oracle_golden.py;
  * the two top-k selections are pinned to outputs of the reference's own ``nnutils.hier_topk`` and of the root selection
    of ``MotifDecoder.decode`` (tests/golden/motif_decode_topk, tests/test_decode_kernel_oracle_cpu.py).

Parameters arrive under the decoder's ``state_dict`` names (``hmpn.E_c.0.weight``, ``hmpn.tree_encoder.rnn.W_z.weight``,
``matchNN.0.weight``, ...), so the layouts ``[x | onehot | s]`` and ``I = H + MAX_POS`` are the module's.
"""
import glob
import os

import numpy as np
import torch

from oracle import ref_decoder as RD
from oracle import ref_encoder as R

MAX_POS = 20
MAX_NB = 12
TOPK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motif_decode_topk")
MIN_GAP = 1e-3          # what every seeded top-k case must keep between consecutive ranked values (see score_rows)


def f64(sd):
    """a state_dict (tensors or arrays) as fp64 tensors"""
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}


def _lt(v):
    return torch.as_tensor(np.asarray(v, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- tree step
def message_input(p, fnode, fmess, rows):
    """[E_c[fnode[src]] | onehot(pos, MAX_POS)] of the messages ``rows``; ``fmess`` is the device table [E, 2] (src, pos)"""
    fm = _lt(fmess)[_lt(rows)]
    emb = p["hmpn.E_c.0.weight"].index_select(0, _lt(fnode)[fm[:, 0]])
    return torch.cat([emb, torch.eye(MAX_POS, dtype=emb.dtype).index_select(0, fm[:, 1])], dim=-1)


def tree_messages(p, rnn, depth, h, c, fnode, fmess, bgraph, rows):
    """sparse_forward of the messages ``rows`` in one call -> (h, c) after it, full [E, H] (c None for GRU)"""
    sub = _lt(rows)
    x, bg = message_input(p, fnode, fmess, rows), _lt(bgraph)[sub]
    h = torch.as_tensor(np.asarray(h)).double()
    if rnn == "GRU":
        return R.gru_sparse_forward(p, "hmpn.tree_encoder.rnn.", h, x, sub, bg, depth), None
    c = torch.as_tensor(np.asarray(c)).double()
    return R.lstm_sparse_forward(p, "hmpn.tree_encoder.rnn.", h, c, x, sub, bg, depth)


def tree_message(p, rnn, depth, h, c, fnode, fmess, bgraph, e):
    """one new message, ``submess = [e]`` -> (h[e], c[e]) after ``depth`` iterations (c[e] None for GRU)"""
    hn, cn = tree_messages(p, rnn, depth, h, c, fnode, fmess, bgraph, [e])
    return hn[e], (None if cn is None else cn[e])


def tree_readout(p, h, fnode, agraph, n):
    """relu(W_o [E_c[fnode[n]] | sum over agraph[n] of h] + b_o): the read-out of mpn_forward for one current node"""
    h = torch.as_tensor(np.asarray(h)).double()
    emb = p["hmpn.E_c.0.weight"].index_select(0, _lt(fnode)[_lt([n])])
    nei = R.gather_rows(h, _lt(agraph)[_lt([n])]).sum(dim=1)
    return torch.relu(R._affine(p, "hmpn.tree_encoder.W_o.0", torch.cat([emb, nei], dim=1)))[0]


# ---------------------------------------------------------------------------------------------- score heads
def mlp(vec, ctx, W1, b1, W2, b2, sigmoid=False):
    """Linear, ReLU, Linear on [vec | ctx] (rows), optionally the sigmoid -> (hidden, out), fp64"""
    t = lambda a: torch.as_tensor(np.asarray(a)).double()      # noqa: E731
    hid = torch.relu(torch.cat([t(vec), t(ctx)], dim=-1) @ t(W1).t() + t(b1))
    out = hid @ t(W2).t() + t(b2)
    return hid, (torch.sigmoid(out) if sigmoid else out)


def assm_score(p, n, icls, nth, z_row):
    """enum_attach + get_assm_score of one prediction with ``n`` candidates -> [n] scores.  The tree-only decoder's
    enum_attach feeds no atom vectors: ref_decoder.enum_attach with zero-width candidate vectors.  The n rows are then one
    row n times, and the decode loop ranks them with a stable sort, so the tie has to be exact: the row is evaluated once
    and repeated (n equal rows of one matrix product need not come out bit-equal -- a BLAS may round its edge rows on
    another path, and on such a host the replayed decodes attach at another atom)."""
    none = torch.zeros(1, 0, dtype=torch.float64)
    v = RD.enum_attach(p, none, torch.zeros(1, len(icls), dtype=torch.long), list(icls), int(nth))
    z = torch.as_tensor(np.asarray(z_row)).double()
    return (R._affine(p, "W_assm", v) * z.unsqueeze(0)).sum(dim=-1).expand(n).clone()


# ---------------------------------------------------------------------------------------------- top k
def _log_softmax(x):
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum())


def _select(v, k, gaps):
    """the best k of v by stable sort (an exact tie goes to the lower index); the gaps between the ranked values of ranks
    0..k (rank k is the first one left out) are appended to ``gaps``"""
    order = np.argsort(-v, kind="stable")
    gaps.extend((-np.diff(v[order[:k + 1]])).tolist())
    return order[:k]


def _min_gap(gaps, ties):
    g = np.asarray(gaps, np.float64)
    if ties:                # exact ties are the subject of the case: the smallest gap among the others
        g = g[g != 0]
    return float(g.min()) if g.size else float("inf")


def _mask(owner, c):
    return np.where(np.asarray(owner) == c, 0.0, -1000.0)


def hier_topk(cls, icls, owner, k, ties=False):
    """nnutils.hier_topk, row by row in fp64 -> (scores [M, k], motifs [M, k], attachments [M, k], smallest gap)"""
    cls, icls = np.asarray(cls, np.float64), np.asarray(icls, np.float64)
    M = cls.shape[0]
    S, C, A, gaps = np.zeros((M, k)), np.zeros((M, k), np.int64), np.zeros((M, k), np.int64), []
    for r in range(M):
        lc = _log_softmax(cls[r])
        top_c = _select(lc, k, gaps)
        sums, sc, sa = np.zeros(k * k), np.zeros(k * k, np.int64), np.zeros(k * k, np.int64)
        for q, c in enumerate(top_c):
            li = _log_softmax(icls[r] + _mask(owner, c))
            top_a = _select(li, k, gaps)
            sums[q * k:(q + 1) * k] = lc[c] + li[top_a]          # flat order q * k + p
            sc[q * k:(q + 1) * k], sa[q * k:(q + 1) * k] = c, top_a
        best = _select(sums, k, gaps)
        S[r], C[r], A[r] = sums[best], sc[best], sa[best]
    return S, C, A, _min_gap(gaps, ties)


def root_topk(cls, icls, owner, k, ties=False):
    """the root of MotifDecoder.decode: the arg-max motif of the raw scores, its raw + mask attachment scores sorted,
    first k, no softmax -> (scores [M, k], motifs [M, k], attachments [M, k], smallest gap)"""
    cls, icls = np.asarray(cls, np.float64), np.asarray(icls, np.float64)
    M = cls.shape[0]
    S, C, A, gaps = np.zeros((M, k)), np.zeros((M, k), np.int64), np.zeros((M, k), np.int64), []
    for r in range(M):
        c = _select(cls[r], 1, gaps)[0]
        v = icls[r] + _mask(owner, c)
        top = _select(v, k, gaps)
        S[r], C[r], A[r] = v[top], c, top
    return S, C, A, _min_gap(gaps, ties)


def heads_topk(p, vecs, ctx, owner, k, root):
    """clsNN and iclsNN on [vecs | ctx], then the root selection or hier_topk -> (scores, motifs, attachments) [M, k]"""
    w = lambda seq: [p[seq + n] for n in (".0.weight", ".0.bias", ".3.weight", ".3.bias")]     # noqa: E731
    cls, icls = mlp(vecs, ctx, *w("clsNN"))[1].numpy(), mlp(vecs, ctx, *w("iclsNN"))[1].numpy()
    return (root_topk if root else hier_topk)(cls, icls, owner, k)[:3]


# ---------------------------------------------------------------------------------------------- a decode backend
class OracleBackend:
    """``ggpm_amd.motif_decode.HipBackend``'s interface in fp64 on the CPU.  It keeps its own mirrors of the tables and
    brings them up to date from the edits alone, as the device does."""

    def __init__(self, dec, src_mol_vecs, B, N, E, beam):
        self.B, self.H, self.L = B, dec.hidden_size, dec.latent_size
        self.p = f64({k: v.detach().cpu().numpy() for k, v in dec.state_dict().items()})
        self.rnn = "LSTM" if hasattr(dec.hmpn.tree_encoder.rnn, "W_f") else "GRU"
        self.depth = dec.hmpn.tree_encoder.rnn.depth
        self.src = [torch.as_tensor(v.detach().cpu().numpy()).double() for v in src_mol_vecs]
        self.fnode = np.zeros(N, np.int64)
        self.tabs = {0: np.zeros((N, MAX_NB), np.int64), 1: np.zeros((E, MAX_NB), np.int64), 2: np.zeros((E, 2), np.int64)}
        self.h, self.c = torch.zeros(E, self.H, dtype=torch.float64), torch.zeros(E, self.H, dtype=torch.float64)
        owner = getattr(dec.vocab, "owner", None)
        self.owner = np.asarray(owner if owner is not None else torch.as_tensor(dec.vocab.mask).argmax(dim=0).numpy())
        self.new_counts()

    def new_counts(self):
        self.cur = {"launches": 0, "d2h": 0, "h2d": 0, "mess": 0, "expand": 0, "scored": 0, "wait_s": 0.0}
        return self.cur

    def _edits(self, tedits):
        for tab, row, slot, v in np.asarray(tedits).reshape(-1, 4):
            if tab == 3:
                assert slot == 0        # (a tree without cgraph queues the motif only)
                self.fnode[row] = v
            else:
                self.tabs[int(tab)][row, slot] = v

    def root(self, k0):
        init = self.src[0] if self.L == self.H else R._affine(self.p, "W_root", self.src[0])
        self.h[1:self.B + 1] = init
        return heads_topk(self.p, init, self.src[1], self.owner, k0, True)

    def phase1(self, tedits, aedits, edges, atoms, nodes, bidx):
        self._edits(tedits)
        read = torch.stack([tree_readout(self.p, self.h, self.fnode, self.tabs[0], int(n)) for n in nodes])
        w = [self.p["topoNN" + n] for n in (".0.weight", ".0.bias", ".3.weight", ".3.bias")]
        return mlp(read, self.src[1][_lt(bidx)], *w, sigmoid=True)[1].reshape(-1).numpy()

    def phase2(self, tedits, nodes, mess, expanding, k):
        self._edits(tedits)
        mess = np.asarray(mess, np.int64).reshape(-1, 2)
        if len(mess):
            self.h, c = tree_messages(self.p, self.rnn, self.depth, self.h, self.c, self.fnode, self.tabs[2], self.tabs[1],
                                      mess[:, 0])
            self.c = self.c if c is None else c
        if not len(expanding):
            return None
        rows = mess[mess[:, 1] >= 0]
        vecs = torch.zeros(len(expanding), self.H, dtype=torch.float64)
        vecs[_lt(rows[:, 1])] = self.h[_lt(rows[:, 0])]
        return heads_topk(self.p, vecs, self.src[1][_lt(expanding)], self.owner, k, False)

    def phase3(self, meta, ids, atoms, n_cand):
        out = np.zeros(n_cand)
        for n, k, nth, b, coff, roff, _ in np.asarray(meta).reshape(-1, 7):
            out[coff:coff + n] = assm_score(self.p, n, ids[roff:roff + k], nth, self.src[2][b]).numpy()
        return out


# ---------------------------------------------------------------------------------------------- seeded inputs
def score_rows(rs, M, n):
    """[M, n] fp32 score rows: a permutation of 0.01 * (0 .. n-1) plus uniform(0, 0.003), centred.  Any two scores of a
    row differ by at least 0.007; Gaussian scores would put near-ties at every rank of a wide vocabulary."""
    out = np.zeros((M, n), np.float32)
    for r in range(M):
        v = rs.permutation(n) * 0.01 + rs.uniform(0.0, 0.003, n)
        out[r] = (v - v.mean()).astype(np.float32)
    return out


def ragged_owner(rs, n_cls, n_icls, cap=None):
    """owner [n_icls] of a ragged, shuffled vocabulary: one motif owns nothing, a quarter of the others one attachment,
    up to an eighth of the rest 18 or more (when ``cap`` and the sizes leave room), the remainder spread at random, no
    motif above ``cap``"""
    order = rs.permutation(n_cls)
    rest = order[1:]                                    # order[0] owns none
    counts = np.zeros(n_cls, np.int64)
    counts[rest] = 1
    left = n_icls - (n_cls - 1)
    assert left >= 0, "fewer attachments than owning motifs"
    cap = n_icls if cap is None else cap
    grow = rest[(n_cls - 1) // 4:]
    for m in grow[:max(1, min(len(grow) // 8, left // 34))]:        # (at most half of what is left goes to these)
        add = max(0, min(left, 17, cap - 1))
        counts[m] += add
        left -= add
    assert left <= int((cap - counts[grow]).sum()), "cap too small"
    while left > 0:
        m = grow[rs.randint(len(grow))]
        if counts[m] < cap:
            counts[m] += 1
            left -= 1
    owner = np.repeat(np.arange(n_cls), counts)
    rs.shuffle(owner)
    return owner.astype(np.int64)


def topk_inputs(n_cls, n_icls, k, seed, M=7, cap=None):
    """the seeded inputs of one top-k case -> (cls [M, n_cls] fp32, icls [M, n_icls] fp32, owner [n_icls])"""
    rs = np.random.RandomState(seed)
    owner = ragged_owner(rs, n_cls, n_icls, cap)
    return score_rows(rs, M, n_cls), score_rows(rs, M, n_icls), owner


# (n_cls, n_icls, k, cap of attachments per motif, seed).  The seeds were found once on the CPU
# (`PYTHONPATH=. python tests/decode_kernel_oracle.py --seeds`): the first for which both restatements keep MIN_GAP at every selection,
# the k x k merge included -- its sums have no floor of their own (2.5e-5 turns up at k = 16), and raw - 1000 has an
# fp32 ulp of 6.1e-5, so the fp32 kernel cannot be asked to rank closer values the way fp64 does.
TOPK_CASES = [
    (12, 36, 5, None, 0),
    (300, 900, 5, None, 0),
    (257, 513, 16, None, 2),
    (700, 2100, 5, None, 1),
    (16, 16, 16, None, 0),
    (40, 130, 16, 15, 3),
]


def find_seed(n_cls, n_icls, k, cap, start=0, tries=20000):
    for seed in range(start, start + tries):
        cls, icls, owner = topk_inputs(n_cls, n_icls, k, seed, cap=cap)
        if min(hier_topk(cls, icls, owner, k)[3], root_topk(cls, icls, owner, k)[3]) >= MIN_GAP:
            return seed
    raise RuntimeError("no seed for %r" % ((n_cls, n_icls, k),))


def tie_case():
    """Hand-made exact ties, k = 5: every motif score equal (motifs 0..4 are chosen, in order); motif 0 owns three equal
    attachment scores at 3, 3 + 64 and 3 + 256 and two equal lower ones at 5 and 5 + 256, motif 1 two equal ones at 4
    and 4 + 256; motifs 2..4 spread their mass, so the merge takes motif 1's pair, then motif 0's triple.  Every other gap is
    wide.  -> (cls [1, 300], icls [1, 600], owner, k, expected {mode: (motifs, attachments)})"""
    n_cls, n_icls, k = 300, 600, 5
    cls = np.zeros((1, n_cls), np.float32)
    owner = 5 + np.arange(n_icls) % (n_cls - 5)
    icls = (-3.0 - 0.01 * np.arange(n_icls)).astype(np.float32)[None, :].copy()
    own = {0: {3: 1.0, 67: 1.0, 259: 1.0, 5: -4.0, 261: -4.0, 70: -6.0},
           1: {4: 0.875, 260: 0.875, 68: -4.0, 132: -5.0, 516: -6.0, 9: -7.0},
           2: {6: 0.75, 300: 0.45, 301: 0.15, 302: -0.15, 303: -0.45, 304: -0.75},
           3: {7: 0.625, 400: 0.575, 401: 0.525, 402: 0.475},       # fewer than k: a masked one follows, by raw score
           4: {8: 0.5625, 410: 0.5125, 411: 0.4625, 412: 0.4125, 413: 0.3625}}
    for m, d in own.items():
        for j, v in d.items():
            owner[j], icls[0, j] = m, v
    expected = {"root": ([0] * 5, [3, 67, 259, 5, 261]), "hier": ([1, 1, 0, 0, 0], [4, 260, 3, 67, 259])}
    return cls, icls, owner.astype(np.int64), k, expected


NB_COUNTS = (0, 1, 3, 11, 12)       # live entries of a neighbour row: none, one, a few, one short of full, full


def neighbour_row(rs, cnt, pool):
    """a MAX_NB-slot row with ``cnt`` distinct ids of ``pool`` in shuffled slots, zeros between them"""
    row = np.zeros(MAX_NB, np.int32)
    row[rs.permutation(MAX_NB)[:cnt]] = rs.choice(pool, size=cnt, replace=False)
    return row


def tree_state(seed, H, N=30, E=60, n_motif=50, n_work=14):
    """A resident decode tree and one launch's work of each kind -> dict of arrays:
    fnode [N], fmess [E, 2] (src, pos), agraph [N, 12], bgraph [E, 12], h / c [E, H] fp32 with row 0 zero;
    ``nodes`` [n_work] to read out and ``mess`` [n_work, 2] = (message, out_row) to compute, out_row -1 for every second
    one and a shuffled row of a 16-row buffer for the others; ``cnt_nodes`` / ``cnt_mess`` the live neighbours of each
    (NB_COUNTS in turn).  No listed message is a neighbour of a listed message; pos is 0, MAX_POS - 1 or random."""
    rs = np.random.RandomState(seed)
    st = {"N": N, "E": E, "H": H}
    st["fnode"] = rs.randint(0, n_motif, N).astype(np.int32)
    st["h"] = (0.5 * rs.standard_normal((E, H))).astype(np.float32)
    st["c"] = (0.5 * rs.standard_normal((E, H))).astype(np.float32)
    st["h"][0] = 0
    st["c"][0] = 0
    fmess = np.stack([rs.randint(1, N, E), rs.randint(0, MAX_POS, E)], axis=1).astype(np.int32)
    listed = rs.choice(np.arange(1, E), size=n_work, replace=False)
    others = np.setdiff1d(np.arange(1, E), listed)
    bgraph = np.stack([neighbour_row(rs, rs.randint(0, MAX_NB + 1), np.arange(1, E)) for _ in range(E)])
    agraph = np.stack([neighbour_row(rs, rs.randint(0, MAX_NB + 1), np.arange(1, E)) for _ in range(N)])
    nodes = rs.choice(np.arange(1, N), size=n_work, replace=False)
    rows = rs.permutation(16)
    mess = []
    for i in range(n_work):
        cnt = NB_COUNTS[i % len(NB_COUNTS)]
        bgraph[listed[i]] = neighbour_row(rs, cnt, others)
        agraph[nodes[i]] = neighbour_row(rs, cnt, np.arange(1, E))
        if i % 3 < 2:
            fmess[listed[i], 1] = (0, MAX_POS - 1)[i % 3]
        mess.append((listed[i], -1 if i % 2 else rows[i // 2]))
    st.update(fmess=fmess, agraph=agraph, bgraph=bgraph, nodes=nodes.astype(np.int32), mess=np.asarray(mess, np.int32),
              cnt_nodes=[NB_COUNTS[i % len(NB_COUNTS)] for i in range(n_work)],
              cnt_mess=[NB_COUNTS[i % len(NB_COUNTS)] for i in range(n_work)])
    return st


_DECODERS = {}


def decoder(rnn, H, L, n_motif, n_attach, seed=5):
    """a real MotifDecoder (CPU, eval) with seeded_state_dict weights, remembered"""
    key = (rnn, H, L, n_motif, n_attach, seed)
    if key not in _DECODERS:
        from decode_fixtures import AtomVocab, state_dict
        from ggpm_amd.motif_decoder import MotifDecoder
        from ggpm_amd.vocab import IndexPairVocab
        if len(_DECODERS) >= 4:
            _DECODERS.clear()
        d = MotifDecoder(IndexPairVocab(n_motif, n_attach, np.arange(n_attach) % n_motif), AtomVocab(), rnn, H, H, L, 1, 1,
                         0.0)
        d.load_state_dict(state_dict(d, [k for k, _ in d.named_parameters()], seed, 0.0), strict=True)
        _DECODERS[key] = d.eval()
    return _DECODERS[key]


# ---------------------------------------------------------------------------------------------- recorded reference
def topk_fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(TOPK_DIR, "*.npz")))


class TopkGolden:
    """one file of tests/golden/motif_decode_topk: meta, owner and the reference's outputs; inputs come from the seed"""

    def __init__(self, name):
        z = np.load(os.path.join(TOPK_DIR, name + ".npz"))
        self.n_cls, self.n_icls, self.k, self.k_root, self.M, self.seed, self.cap = [int(v) for v in z["meta"]]
        self.owner, self.hier, self.root = z["owner"], z["hier"], z["root"]
        cap = self.cap if self.cap > 0 else None
        self.cls, self.icls, owner = topk_inputs(self.n_cls, self.n_icls, self.k, self.seed, self.M, cap)
        assert np.array_equal(owner, self.owner), "the seeded generator no longer makes the recorded owner table"

    @staticmethod
    def split(out, k):
        """[M, 3k] -> (scores, motifs, attachments)"""
        return out[:, :k], out[:, k:2 * k].astype(np.int64), out[:, 2 * k:].astype(np.int64)


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        for n_cls, n_icls, k, cap, _ in TOPK_CASES:
            print((n_cls, n_icls, k, cap), "seed", find_seed(n_cls, n_icls, k, cap))
