"""Dropout masks of a training step that the tests know independently of the code under test, and the oracle's ``drop``
hook that applies them (oracle/ref_decoder.decoder_forward, ref_encoder.inc_hier_forward).

Two kinds of site:
  * sites the HIP code masks itself with ggpm_dropout (include/ggpm_hip.h): the encoder's seven (sites 0-6, the drivers'
    masks), the decoder's atom-level W_o (atom_decode.py) and the property heads (sites 16-23).  Their masks are restated
    with golden_utils.dropout_keep from the pinned seed, row for row.
  * sites that reach torch's own nn.Dropout modules (the two tree-side decoder levels, E_assm, the score heads, the atom
    level's W_o in the step-by-step forms).  The test swaps each module for an ``InjectedDropout`` that applies a
    PER-COLUMN keep vector, the same for every row: the forms of the decoder call these modules with different row orders
    and numbers of calls (one call over all visits, or one per decode step), so a per-column mask is reproduced without
    a row mapping.
"""
import numpy as np
import torch

from golden_utils import dropout_keep

ENC_SITES = {"E_i": 0, "E_c": 1, "graph_encoder.W_o": 2, "W_i": 3, "inter_encoder.W_o": 4, "W_c": 5,
             "tree_encoder.W_o": 6}

# oracle site -> the decoder's nn.Dropout module it is (E_assm IS hmpn.E_i: the same module, the same column mask)
COLUMN_SITES = {"E_i": "hmpn.E_i.1", "E_assm": "hmpn.E_i.1", "E_c": "hmpn.E_c.1", "W_i": "hmpn.W_i.2",
                "W_c": "hmpn.W_c.2", "inter_encoder.W_o": "hmpn.inter_encoder.W_o.2",
                "tree_encoder.W_o": "hmpn.tree_encoder.W_o.2", "graph_encoder.W_o": "hmpn.graph_encoder.W_o.2",
                "topoNN.2": "topoNN.2", "clsNN.2": "clsNN.2", "iclsNN.2": "iclsNN.2"}
MODULES = sorted(set(COLUMN_SITES.values()))
COLUMN_SEED = (2718281, 3141592)        # the test's own mask stream for the per-column masks


def padded(H):
    return (H + 15) // 16 * 16


def scaled(keep, p):
    return keep.astype(np.float32) / np.float32(1.0 - p)


def encoder_masks(n_tree_nodes, n_graph_nodes, H, p, seed):
    """{oracle key: [rows, H] scaled mask} of the encoder drivers' seven sites (ref_encoder.hier_encoder_forward masks)."""
    rows = lambda k: n_graph_nodes if k == "graph_encoder.W_o" else n_tree_nodes
    return {k: torch.from_numpy(scaled(dropout_keep(rows(k), H, p, seed[0], seed[1], s), p)) for k, s in ENC_SITES.items()}


def atom_row_masks(aoff, H, p, seed):
    """Per decode step t the [atoms of step t, H] scaled mask of the atom level's W_o rows (row j = st["atoms"][j]):
    one call at site 0 over the rows of all steps (step t's rows start at aoff[t])."""
    m = dropout_keep(aoff[-1], H, p, seed[0], seed[1], 0)
    return [scaled(m[aoff[t]:aoff[t + 1]], p) for t in range(len(aoff) - 1)]


def column_masks(H, p):
    """{module path: [Hp] scaled per-column keep vector} (float32, CPU)."""
    return {m: torch.from_numpy(scaled(dropout_keep(1, padded(H), p, COLUMN_SEED[0], COLUMN_SEED[1], 100 + i)[0], p))
            for i, m in enumerate(MODULES)}


class InjectedDropout(torch.nn.Dropout):
    """nn.Dropout (same ``p``, same training-mode semantics, so the product's gating sees an active dropout) that applies
    a fixed per-column mask and counts its calls and rows."""

    def __init__(self, p, cols):
        super().__init__(p)
        self.cols = cols
        self.calls = 0
        self.rows = 0

    def forward(self, x):
        if not self.training or self.p == 0:
            return x
        self.calls += 1
        self.rows += x.shape[0]
        return x * self.cols[:x.shape[-1]].to(device=x.device, dtype=x.dtype)


def inject(decoder, p, H):
    """Replace the decoder's nn.Dropout modules by InjectedDropout ones -> {module path: module}."""
    cols = column_masks(H, p)
    out = {}
    for path in MODULES:
        *parent, last = path.split(".")
        seq = decoder.get_submodule(".".join(parent))
        assert isinstance(seq[int(last)], torch.nn.Dropout), path
        seq[int(last)] = out[path] = InjectedDropout(p, cols[path].to(next(decoder.parameters()).device))
    return out


def oracle_drop(H, p, atom_rows=None, counts=None):
    """The oracle's ``drop(site, x, step)``: the per-column masks of ``column_masks`` at every site, except the atom level's
    W_o when ``atom_rows`` (from atom_row_masks) is given.  ``counts``: dict site -> rows seen, filled in."""
    cols = column_masks(H, p)

    def drop(site, x, step):
        if counts is not None:
            counts[site] = counts.get(site, 0) + x.shape[0]
        if site == "graph_encoder.W_o" and atom_rows is not None:
            m = atom_rows[step]
            assert m.shape == tuple(x.shape), (site, step, m.shape, tuple(x.shape))
            return x * torch.from_numpy(m).to(x.dtype)
        return x * cols[COLUMN_SITES[site]][:x.shape[-1]].to(x.dtype)
    return drop
