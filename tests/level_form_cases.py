"""The forms a GRU / LSTM level call can take at the configured hidden sizes, as a table of test cases, and their inputs.

A level call's launch geometry is decided per call (csrc/tile_mma.h: ggpm_tiles_per_group; csrc/level_host.h: level_plan,
fwd_step, bwd_step over the cell descriptions of csrc/mpn_gru.hip and csrc/mpn_lstm.hip) and reported by
``ggpm_level_form_query``.  A case names one call and the
form the table expects it to take, reduced to ``(tg, groups, gate_mode, rt2, fuse_fwd, fuse_bwd)``:
tests/test_level_forms_cpu.py holds the table to the lattice the query spans (every reachable form has a case; every case
has the form it states), tests/test_gpu_level_forms.py runs every case against the fp64 oracle.
"""
from collections import namedtuple

import numpy as np

I, K = 20, 4          # input width and predecessor slots of every case
HIDDEN = (250, 300, 600)        # the hidden sizes of the shipped configurations

# form: (tg, groups, gate_mode, rt2, fuse_fwd, fuse_bwd); E1 counts the pad row; ms: recomputed rows of a sparse call
Case = namedtuple("Case", "cell H E1 depth form sparse ms")


def _dense(cell, H, E1, form, depth=2):
    return Case(cell, H, E1, depth, form, False, 0)


def _sparse(cell, H, E1, form, depth=2):
    return Case(cell, H, E1, depth, form, True, E1 // 4)        # about a quarter of the rows recomputed


def _groups(tg, groups):
    """a column-grouped form: fp32 MFMA, one row tile, B launches"""
    return (tg, groups, 0, 0, 0, 0)


# H -> [(E1, (tg, groups), depth)]: the lower end of every class (the smallest E1 that takes it; 40 for the first), and the
# upper end (E1 a multiple of 16: the last row tile full) of the two-group classes.  Depth 3 on the H = 600 two-group class:
# two full gate-product steps on the path where a wave owns two tiles of a group.
_GROUPED = {
    250: [(40, (4, 4), 2), (1025, (6, 3), 2), (1361, (8, 2), 2), (2048, (8, 2), 2)],
    300: [(40, (4, 5), 2), (817, (5, 4), 2), (1025, (7, 3), 2), (1361, (10, 2), 2), (2048, (10, 2), 2)],
    600: [(40, (4, 10), 2), (401, (5, 8), 2), (513, (6, 7), 2), (577, (7, 6), 2), (673, (8, 5), 2), (817, (10, 4), 2),
          (1025, (13, 3), 2), (1361, (19, 2), 3), (2048, (19, 2), 3)],
}
# the single-group form (E1 >= 2049) of a dense call: split operands with everything fused where the images fit the LDS;
# at H = 600 the GRU keeps split operands without room for a fused phase, the LSTM falls back to fp32 MFMA with qf' fused
_SINGLE_DENSE = {("GRU", 250): (16, 1, 2, 0, 1, 1), ("LSTM", 250): (16, 1, 2, 0, 1, 1),
                 ("GRU", 300): (19, 1, 2, 0, 1, 1), ("LSTM", 300): (19, 1, 2, 0, 1, 1),
                 ("GRU", 600): (38, 1, 2, 0, 0, 0), ("LSTM", 600): (38, 1, 0, 0, 1, 0)}
# ... and of a sparse call (always fp32 MFMA): the full-level form of the decode steps
_SINGLE_SPARSE = {250: (16, 1, 0, 0, 1, 1), 300: (19, 1, 0, 0, 1, 1), 600: (38, 1, 0, 0, 1, 0)}

DENSE = []
for _cell in ("GRU", "LSTM"):
    for _H in HIDDEN:
        DENSE += [_dense(_cell, _H, E1, _groups(*cls), depth) for E1, cls, depth in _GROUPED[_H]]
        DENSE.append(_dense(_cell, _H, 2049, _SINGLE_DENSE[_cell, _H]))
# the natural two-row-tile form (512 row tiles and more; no prefer_narrow)
DENSE.append(_dense("GRU", 300, 8177, (19, 1, 0, 1, 0, 0)))

# sparse calls: the class of E1 = 450 (tg 4 or 5), two groups, one group
SPARSE_E1 = (450, 1361, 2049)
SPARSE = []
for _cell in ("GRU", "LSTM"):
    for _H in HIDDEN:
        _cls = {E1: cls for E1, cls, _ in _GROUPED[_H]}
        SPARSE += [_sparse(_cell, _H, 450, _groups(*(_cls[401] if _H == 600 else _cls[40]))),
                   _sparse(_cell, _H, 1361, _groups(*_cls[1361])), _sparse(_cell, _H, 2049, _SINGLE_SPARSE[_H])]

# The accepted hidden-size limits (include/ggpm_hip.h: "Accepted hidden sizes").  GRU H = 1264 (79 tiles): 20 groups; tg 16,
# every wave owns one tile; two groups, three tiles per wave; one group, five tiles per wave, nothing fused.  GRU H = 840 /
# 850 (Hp = 848 / 864): the last size with q' fused into a single-group forward and the first without.  LSTM H = 848 (53
# tiles): 14 groups; tg 18, two tiles per wave, three groups; one group.
GRU_MAX_H, LSTM_MAX_H = 1264, 848
LIMIT_DENSE = [_dense("GRU", 1264, 40, _groups(4, 20)), _dense("GRU", 1264, 673, _groups(16, 5)),
               _dense("GRU", 1264, 1361, _groups(40, 2)), _dense("GRU", 1264, 2049, (79, 1, 0, 0, 0, 0)),
               _dense("GRU", 840, 2049, (53, 1, 0, 0, 1, 0)), _dense("GRU", 850, 2049, (54, 1, 0, 0, 0, 0)),
               _dense("LSTM", 848, 40, _groups(4, 14)), _dense("LSTM", 848, 1025, _groups(18, 3)),
               _dense("LSTM", 848, 2049, (53, 1, 0, 0, 1, 0))]
LIMIT_SPARSE = [_sparse("LSTM", 848, 450, _groups(7, 8))]


def case_id(c):
    return "%s-H%d-E%d-d%d%s" % (c.cell, c.H, c.E1, c.depth, "-sparse" if c.sparse else "")


def reduced(form):
    """a ggpm_level_form (functional.LevelForm) as the tuple the table states"""
    return (form.tg, form.groups, form.gate_mode, form.rt2, form.fuse_fwd, form.fuse_bwd)


def query(case, training=True):
    """-> the LevelForm of the case's call under default options (None: refused)"""
    from ggpm_amd import functional as F_
    return F_.level_form(case.cell == "LSTM", case.E1, case.H, sparse=case.sparse, training=training)


def _seed(case):
    return 7 * case.E1 + case.H + 3 * case.depth + (1 if case.cell == "LSTM" else 0)


def random_level(rs, E, n_in, k_max=K):
    """A random predecessor table as tests/test_gpu_parity.py draws them (every message 0 .. k_max distinct predecessors
    among 1 .. E, zero padded; row 0 is the pad message), drawn for all rows at once, and inputs [E + 1, n_in]."""
    cand = rs.randint(1, E + 1, size=(E + 1, k_max))
    for j in range(1, k_max):            # a repeated id becomes an empty slot
        cand[:, j] = np.where((cand[:, :j] == cand[:, j:j + 1]).any(axis=1), 0, cand[:, j])
    keep = np.arange(k_max)[None, :] < rs.randint(0, k_max + 1, size=(E + 1, 1))
    bgraph = np.zeros((E + 1, k_max + 1), dtype=np.int64)
    bgraph[:, :k_max] = np.where(keep, cand, 0)
    bgraph[0] = 0
    bgraph[:, :k_max] = -np.sort(-bgraph[:, :k_max], axis=1)      # ids first, padding behind them
    x = rs.standard_normal((E + 1, n_in)).astype(np.float32)
    return x, bgraph


def weights(case):
    from ggpm_amd.params import rnn_param_shapes, seeded_state_dict
    return seeded_state_dict(rnn_param_shapes(case.cell, I, case.H), seed=_seed(case))


def dense_inputs(case):
    """-> x [E1, I], bgraph [E1, K + 1], the cotangent on h [E1, H]"""
    rs = np.random.RandomState(_seed(case))
    x, bgraph = random_level(rs, case.E1 - 1, I)
    return x, bgraph, rs.standard_normal((case.E1, case.H)).astype(np.float32)


def sparse_case_inputs(case):
    """golden_utils.sparse_inputs of the case: h, c, submess, x, bgraph, the cotangents on (h, c)"""
    from golden_utils import sparse_inputs
    return sparse_inputs(case.E1, I, case.H, case.ms, K, _seed(case))
