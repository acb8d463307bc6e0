"""A synthetic molecule-assembly object (a "graph batch") for ``MotifDecoder.decode`` without rdkit.

``MotifDecoder.decode`` (reference ggpm/decoder.py:901-1095) reaches chemistry only through the object it builds at
ggpm/decoder.py:908 (``IncGraph``) and the anchor labels it computes at :1072.  ``SynthGraphBatch`` has the same methods
with deterministic rules -- those of :func:`ggpm_amd.synth.random_molecule` -- so that decode runs, and can be pinned
against the reference, anywhere:

  * attachment id j (``'a<j>'``, ``IndexPairVocab.get_ismiles``) is a fragment of shape ``(bond, 5-ring, 6-ring)[j % 3]``
    whose atom i has the label ``ATOMS[(j // 3 + i) % 4]``; the motif id plays no part;
  * a child shares one atom with its parent (its attach point 0), except a ring fragment with ``j % 4 == 3``, which shares
    a bond: attach points 0 and 1 on two bonded parent atoms (the two-atom attachment of fused rings);
  * candidates (``get_assm_cands``): the atoms of the parent cluster that no attachment has used, in cluster order, as
    1-tuples; for two attach points the bonded pairs of such atoms, in ring order.  An exhausted parent has none;
  * valence: an atom carries at most 4 bonds (C), 3 (N) or 2 (O, S); ``try_add_mol`` refuses an attachment that would
    exceed it at a parent atom (a ring child adds 2 bonds at its one shared atom, a bond child 1, a fused ring 1 at each);
  * anchor labels (``anchor_label`` and the second result of ``get_assm_cands``): the fragment's own ``'a<j>'`` per
    attach point;
  * ``get_mol()``: per molecule the string ``'<atom labels>|<i>-<j>,...'``: its atoms in the order they were added, its
    bonds as sorted pairs of those positions.
Together the rules give one candidate (bond parents), several (ring parents), none (exhausted parents) and refusals (N,
O and S atoms), so decode meets every branch of the reference's loop: the fall-through to the next candidate and beam
entry, and the forced backtrack.  Atom ids are global over the batch and start at 1, as IncGraph's do.

``SynthHierGraphBatch`` adds what ``HierMPNDecoder.decode`` (reference ggpm/decoder.py:303-472) reads besides: the atom-level
tables ``fnode``, ``fmess``, ``agraph`` and ``bgraph`` of ``IncBase`` (reference ggpm/inc_graph.py:10-57), written in place
by ``add_mol`` slot for slot as ``IncGraph.add_mol`` (:136-187) writes them, and returned by ``get_tensors()`` as host
tensors:
  * an atom's feature is the one-hot of ``avocab[(symbol, 0)]`` (an unknown symbol is the vocabulary's ``KeyError``).  It is
    handed to ``add_node(feature)``, which -- as ``IncBase.add_node`` (:23-29) -- does not store it: the ``fnode`` rows stay
    zero in the reference's decode, and so they do here;
  * a message row is ``[one-hot source atom | one-hot bond type | one-hot(nth_child if the destination atom is attached,
    else 0)]``; the source symbol is the fragment's own label of that atom, as the reference reads it from the fragment;
  * bond types: the bond of a two-atom fragment is type 0, every ring bond type 1;
  * both directions of a new bond are added, (a1, a2) then (a2, a1), in the fragment's bond order (ring order, the closing
    bond last); a bond that exists already (the shared bond of a fused ring) is not added again;
  * ``add_mol`` returns *directed* message ids, two per bond of the fragment, existing bonds included.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

ATOMS = ("C", "N", "O", "S")
VALENCE = {"C": 4, "N": 3, "O": 2, "S": 2}


def fragment(ismiles):
    """(size, atom labels, number of attach points) of the fragment an attachment label ``'a<j>'`` names."""
    j = int(str(ismiles)[1:])
    size = (2, 5, 6)[j % 3]
    labels = [ATOMS[(j // 3 + i) % len(ATOMS)] for i in range(size)]
    return size, labels, (2 if size > 2 and j % 4 == 3 else 1)


def anchor_label(ismiles, point):
    """The anchor label of attach point ``point`` (what get_anchor_smiles gives the reference at decoder.py:1072)."""
    return str(ismiles)


class SynthGraphBatch:
    """IncGraph's constructor and the methods ``MotifDecoder.decode`` calls (see the module docstring for the rules)."""

    def __init__(self, vocab, avocab, batch_size, max_nodes=100, max_edges=300, node_fdim=0, edge_fdim=0, max_nb=10):
        self.vocab, self.avocab, self.batch_size = vocab, avocab, batch_size
        self.max_edges, self.edge_fdim = max_edges, edge_fdim
        self.label = [None]                 # atom 0 is the pad atom
        self.degree = [0]
        self.owner = [-1]                   # molecule of every atom
        self.bonds = {}                     # (a, b), a < b -> bond id (from 1)
        self.batch = defaultdict(list)      # molecule -> its atoms in the order they were added
        self.mol_bonds = defaultdict(list)  # molecule -> its bonds (a, b)
        self._mol = {}                      # get_mol strings of the molecules no add_mol changed since

    anchor_label = staticmethod(anchor_label)

    def _bond(self, a, b):
        key = (a, b) if a < b else (b, a)
        if key not in self.bonds:
            self.bonds[key] = len(self.bonds) + 1
            self.degree[a] += 1
            self.degree[b] += 1
            self.mol_bonds[self.owner[a]].append(key)
        return self.bonds[key]

    def add_mol(self, bid, ismiles, inter_label, nth_child):
        """-> (the fragment's atoms, its bond ids, the parent atoms it shares in attach-point order)"""
        size, labels, _ = fragment(ismiles)
        shared = {int(p): int(a) for a, p in inter_label}
        atoms = []
        for i in range(size):
            if i in shared:
                atoms.append(shared[i])
                continue
            self.label.append(labels[i])
            self.degree.append(0)
            self.owner.append(bid)
            atoms.append(len(self.label) - 1)
            self.batch[bid].append(atoms[-1])
        ring = [(atoms[i], atoms[i + 1]) for i in range(size - 1)] + ([(atoms[-1], atoms[0])] if size > 2 else [])
        bonds = [self._bond(a, b) for a, b in ring]
        self._mol.pop(bid, None)
        return atoms, bonds, [shared[p] for p in sorted(shared)]

    def get_assm_cands(self, cluster, used, ismiles):
        """-> (candidate tuples of parent atoms, anchor labels, attach points); changes nothing"""
        _, _, npts = fragment(ismiles)
        if npts == 1:
            cands = [(a,) for a in cluster if a not in used]
        else:
            n = len(cluster)
            pairs = [(cluster[i], cluster[(i + 1) % n]) for i in range(n if n > 2 else 1)]
            cands = [(a, b) for a, b in pairs if a not in used and b not in used]
        return cands, [anchor_label(ismiles, p) for p in range(npts)], list(range(npts))

    def try_add_mol(self, bid, ismiles, inter_label):
        size, _, npts = fragment(ismiles)
        need = 1 if size == 2 or npts == 2 else 2
        return all(self.degree[a] + need <= VALENCE[self.label[a]] for a, _ in inter_label)

    def get_mol(self):
        out = [None] * len(self.batch)
        for bid, atoms in self.batch.items():
            s = self._mol.get(bid)
            if s is None:
                pos = {a: i for i, a in enumerate(atoms)}
                bonds = sorted(tuple(sorted((pos[a], pos[b]))) for a, b in self.mol_bonds[bid])
                s = self._mol[bid] = "".join(self.label[a] for a in atoms) + "|" + ",".join("%d-%d" % p for p in bonds)
            out[bid] = s
        return out

    def get_tensors(self):
        """IncGraph's (fnode, fmess, agraph, bgraph, scope) as far as the tree-only decode reads them: the row count of
        fmess (the reference sizes a message state it never uses from it)."""
        return None, torch.zeros(self.max_edges * self.batch_size, max(self.edge_fdim, 1)), None, None, None


NUM_BOND_TYPES = 4      # len(MolGraph.BOND_LIST)
MAX_POS = 20            # MolGraph.MAX_POS


class SynthAtomVocab:
    """The reference's ``common_atom_vocab`` as far as the synthetic fragments need it: 38 entries, the neutral C, N, O
    and S at their places in that table."""

    IDS = {("C", 0): 5, ("N", 0): 21, ("O", 0): 24, ("S", 0): 30}

    def size(self):
        return 38

    def __getitem__(self, key):
        return self.IDS[key]


class SynthHierGraphBatch(SynthGraphBatch):
    """``SynthGraphBatch`` with IncGraph's atom-level tables (see the module docstring).  ``get_assm_cands``,
    ``try_add_mol``, ``get_mol``, ``anchor_label`` and the fragment rules are SynthGraphBatch's."""

    def __init__(self, vocab, avocab, batch_size, node_fdim=0, edge_fdim=0, max_nodes=100, max_edges=300, max_nb=10):
        super().__init__(vocab, avocab, batch_size, max_nodes, max_edges, node_fdim, edge_fdim, max_nb)
        self.max_nb = max_nb
        # numpy tables (scalar writes cost a tenth of a tensor's); get_tensors() hands out tensors over the same memory
        self._fnode = np.zeros((max_nodes * batch_size, node_fdim), np.float32)
        self._fmess = np.zeros((max_edges * batch_size, edge_fdim), np.float32)
        self._agraph = np.zeros((max_edges * batch_size, max_nb), np.int64)      # sized by edges, as IncBase's
        self._bgraph = np.zeros((max_edges * batch_size, max_nb), np.int64)
        self.fnode, self.fmess = torch.from_numpy(self._fnode), torch.from_numpy(self._fmess)
        self.agraph, self.bgraph = torch.from_numpy(self._agraph), torch.from_numpy(self._bgraph)
        self.preds, self.succs = [[]], [[]]
        self.edge_dict = {None: 0}

    def get_tensors(self):
        """IncGraph's (fnode, fmess, agraph, bgraph, scope): host tensors that ``add_mol`` writes in place"""
        return self.fnode, self.fmess, self.agraph, self.bgraph, None

    def get_atom_feature(self, symbol):
        f = np.zeros(self.avocab.size(), np.float32)
        f[self.avocab[(symbol, 0)]] = 1
        return f

    def get_mess_feature(self, symbol, bond_type, nth_child):
        n = self.avocab.size()
        f = np.zeros(n + NUM_BOND_TYPES + MAX_POS, np.float32)
        f[:n][self.avocab[(symbol, 0)]] = 1
        f[n:n + NUM_BOND_TYPES][bond_type] = 1
        f[n + NUM_BOND_TYPES:][nth_child] = 1
        return f

    def add_node(self, feature=None):
        """IncBase.add_node: the feature is not stored"""
        self.preds.append([])
        self.succs.append([])
        return len(self.preds) - 1

    def add_edge(self, i, j, feature=None):
        """IncBase.add_edge"""
        if (i, j) in self.edge_dict:
            return self.edge_dict[(i, j)]
        self.preds[j].append(i)
        self.succs[i].append(j)
        self.edge_dict[(i, j)] = idx = len(self.edge_dict)
        self._agraph[j, len(self.preds[j]) - 1] = idx
        if feature is not None:
            self._fmess[idx, :len(feature)] = feature
        in_edges = [self.edge_dict[(k, i)] for k in self.preds[i] if k != j]
        self._bgraph[idx, :len(in_edges)] = in_edges
        for k in self.succs[j]:
            if k != i:
                self._bgraph[self.edge_dict[(j, k)], len(self.preds[j]) - 2] = idx
        return idx

    def add_mol(self, bid, ismiles, inter_label, nth_child):
        """-> (the fragment's atoms, its directed message ids, the parent atoms it shares in attach-point order)"""
        size, labels, _ = fragment(ismiles)
        shared = {int(p): int(a) for a, p in inter_label}
        atoms, attached = [], []
        for i in range(size):
            if i in shared:
                atoms.append(shared[i])
                attached.append(shared[i])
                continue
            feature = self.get_atom_feature(labels[i])
            self.label.append(labels[i])
            self.degree.append(0)
            self.owner.append(bid)
            idx = len(self.label) - 1
            assert idx == self.add_node(feature)
            atoms.append(idx)
            self.batch[bid].append(idx)
        ring = [(i, i + 1) for i in range(size - 1)] + ([(size - 1, 0)] if size > 2 else [])
        bond_type = 0 if size == 2 else 1
        bonds = []
        for p, q in ring:
            a1, a2 = atoms[p], atoms[q]
            if ((a1, a2) if a1 < a2 else (a2, a1)) not in self.bonds:
                self._bond(a1, a2)
                self.add_edge(a1, a2, self.get_mess_feature(labels[p], bond_type, nth_child if a2 in attached else 0))
                self.add_edge(a2, a1, self.get_mess_feature(labels[q], bond_type, nth_child if a1 in attached else 0))
            bonds.extend([self.edge_dict[(a1, a2)], self.edge_dict[(a2, a1)]])
        self._mol.pop(bid, None)
        return atoms, bonds, [shared[p] for p in sorted(shared)]
