"""The forms a GRU / LSTM level call can take at the configured hidden sizes, as a table of test cases, and their inputs.

A level call's launch geometry is decided per call (csrc/tile_mma.h: ggpm_tiles_per_group; csrc/level_host.h: level_plan,
fwd_step, bwd_step over the cell descriptions of csrc/mpn_gru.hip and csrc/mpn_lstm.hip) and reported by
``ggpm_level_form_query``.  A case names one call and the
form the table expects it to take, reduced to ``(tg, groups, gate_mode, rt2, fuse_fwd, fuse_bwd)``:
tests/test_level_forms_cpu.py holds the table to the lattice the query spans (every reachable form has a case; every case
has the form it states), tests/test_gpu_level_forms.py runs every case against the fp64 oracle.

``OPT_DENSE`` / ``OPT_SPARSE`` hold the forms a call reaches only through ``ggpm_level_opts.gate_dtype`` and
``prefer_narrow``; their forms carry ``st16`` as a seventh entry (``reduced_opt``), and
tests/test_gpu_level_option_forms.py runs them.
"""
from collections import namedtuple

import numpy as np

I, K = 20, 4          # input width and predecessor slots of every case
HIDDEN = (250, 300, 600)        # the hidden sizes of the shipped configurations

# form: (tg, groups, gate_mode, rt2, fuse_fwd, fuse_bwd); E1 counts the pad row; ms: recomputed rows of a sparse call;
# gate_dtype (0 .. 3), prefer_narrow (0 / 1): the call's ggpm_level_opts (the option cases; their form ends in st16)
Case = namedtuple("Case", "cell H E1 depth form sparse ms gate_dtype prefer_narrow", defaults=(0, 0))


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

# ---- the forms only options reach (training calls; DESIGN.md 5.1 counts them): one case per form, at the lower end of its
# class -- the smallest E1 that takes it, 40 for the first class, 6144 for bf16 storage, 8177 for the two-row-tile forms a
# call takes by its size -- and at the depth _GROUPED gives the class.  (gate_dtype, prefer_narrow) is the setting a
# product path uses where several reach the form: the module attribute for the gate dtype, prefer_narrow for two row tiles.
_TILES = {250: 16, 300: 19, 600: 38}
# H -> [(E1, (tg, groups), depth)] of every class: the grouped ones from their lower end, then the single group
_CLASSES = {H: [g for g in _GROUPED[H] if g[0] != 2048] + [(2049, (_TILES[H], 1), 2)] for H in HIDDEN}
# what a single-group call fuses under gate modes 0 and 1 (forward, backward); a column-grouped call fuses nothing
_SINGLE_FUSE = {("GRU", 250): (1, 1), ("GRU", 300): (1, 1), ("GRU", 600): (1, 0),
                ("LSTM", 250): (1, 1), ("LSTM", 300): (1, 1), ("LSTM", 600): (1, 0)}
# the hidden sizes at which a cell has two-row-tile kernels that fit the LDS / split images that fit beside its tiles
_RT2_H = {"GRU": (250, 300, 600), "LSTM": (250, 300)}
_SPLIT_H = {"GRU": (250, 300, 600), "LSTM": (250, 300)}
STORAGE_H, STORAGE_E1, RT2_E1 = (300, 600), 6144, 8177      # bf16 storage: E1 >= 6144 at these H; 511 * 16 + 1 rows


def _opt(cell, H, E1, depth, form, gate_dtype, prefer_narrow):
    return Case(cell, H, E1, depth, form, False, 0, gate_dtype, prefer_narrow)


OPT_DENSE = []
for _cell in ("GRU", "LSTM"):
    for _H in HIDDEN:
        _ff, _fb = _SINGLE_FUSE[_cell, _H]
        for _E1, (_tg, _g), _d in _CLASSES[_H]:
            _one = _g == 1
            _fuse = (_ff, _fb) if _one else (0, 0)
            # bf16 operands, one row tile, fp32 storage (module.gate_dtype = "bf16")
            OPT_DENSE.append(_opt(_cell, _H, _E1, _d, (_tg, _g, 1, 0) + _fuse + (0,), 1, 0))
            if _H in _RT2_H[_cell]:
                # fp32 MFMA on two row tiles, forced (prefer_narrow).  The GRU's single group: a default call takes this form
                # from 8177 rows, where DENSE holds it at H = 300 only -- H = 250 / 600 stand here, at 2049 rows.
                if not (_cell == "GRU" and _one and _H == 300):
                    OPT_DENSE.append(_opt(_cell, _H, _E1, _d, (_tg, _g, 0, 1, 0, 0, 0), 0, 1))
                # bf16 operands on two row tiles (GRU only), forced -- but the single group of H = 250, which a GRU level of
                # 8177 rows takes by itself (no bf16 storage at that size)
                if _cell == "GRU" and not (_one and _H not in STORAGE_H):
                    OPT_DENSE.append(_opt(_cell, _H, _E1, _d, (_tg, _g, 1, 1, 0, 0, 0), 1, 1))
            if _one and (_cell, _H) != ("LSTM", 600):
                # fp32 MFMA where the default splits (gate_dtype 2); the LSTM at H = 600 has no room to split anyway
                OPT_DENSE.append(_opt(_cell, _H, _E1, _d, (_tg, 1, 0, 0) + _fuse + (0,), 2, 0))
            if not _one and _H in _SPLIT_H[_cell]:
                # split operands on a column-grouped form (gate_dtype 3)
                OPT_DENSE.append(_opt(_cell, _H, _E1, _d, (_tg, _g, 2, 0, 0, 0, 0), 3, 0))
        if _H in STORAGE_H:      # bf16 operands + bf16 storage
            OPT_DENSE.append(_opt(_cell, _H, STORAGE_E1, 2, (_TILES[_H], 1, 1, 0, _ff, _fb, 1), 1, 0))
        if _cell == "GRU":       # the natural two-row-tile form under bf16: with bf16 storage where the level has it
            OPT_DENSE.append(_opt(_cell, _H, RT2_E1, 2, (_TILES[_H], 1, 1, 1, 0, 0, int(_H in STORAGE_H)), 1, 0))

# sparse calls under gate_dtype 1 and 3, on the three classes of SPARSE_E1 (a sparse call never takes two row tiles and
# never stores bf16).  gate_dtype 3: the single group fuses what the dense default does on split operands; the LSTM at
# H = 600 has no room for the images and keeps the default form, which SPARSE holds.
OPT_SPARSE = []
for _c in SPARSE:
    _tg, _g, _, _, _ff, _fb = _c.form
    OPT_SPARSE.append(_c._replace(form=(_tg, _g, 1, 0, _ff, _fb, 0), gate_dtype=1))
    _split = _SINGLE_DENSE[_c.cell, _c.H] if _g == 1 else (_tg, _g, 2, 0, 0, 0)
    if _split[2] == 2 and _c.H in _SPLIT_H[_c.cell]:
        OPT_SPARSE.append(_c._replace(form=_split + (0,), gate_dtype=3))


def case_id(c):
    return "%s-H%d-E%d-d%d%s%s%s" % (c.cell, c.H, c.E1, c.depth, "-sparse" if c.sparse else "",
                                     "-dt%d" % c.gate_dtype if c.gate_dtype else "", "-narrow" if c.prefer_narrow else "")


def reduced(form):
    """a ggpm_level_form (functional.LevelForm) as the tuple the table states"""
    return (form.tg, form.groups, form.gate_mode, form.rt2, form.fuse_fwd, form.fuse_bwd)


def reduced_opt(form):
    """... with st16: what the option tables state"""
    return reduced(form) + (form.st16,)


def level_opts(case, **fields):
    """-> the functional.LevelOpts of the case's call (None: all defaults)"""
    from ggpm_amd import functional as F_
    if not (case.gate_dtype or case.prefer_narrow or fields):
        return None
    return F_.LevelOpts(gate_dtype=case.gate_dtype, prefer_narrow=case.prefer_narrow, **fields)


def query(case, training=True):
    """-> the LevelForm of the case's call under its options (None: refused)"""
    from ggpm_amd import functional as F_
    return F_.level_form(case.cell == "LSTM", case.E1, case.H, sparse=case.sparse, training=training, opts=level_opts(case))


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
