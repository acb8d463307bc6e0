"""CPU: the case tables of tests/row_op_cases.py against the constants of csrc/graph.hip and the dispatch conditions of
csrc/gather.hip, and the host restatements against plain Python loops on tiny inputs.

The GPU cases (tests/test_row_ops_gpu.py) are built for the sort tiers and launch forms as the source has them today: a list
exactly at every boundary and one exactly past it.  The constants are read from the source here, so that moving one fails this
test instead of leaving the GPU cases on the wrong tier without anybody noticing."""
import os
import re

import numpy as np
import torch

import row_op_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "ggpm_amd", "csrc", name)) as f:
        return f.read()


def _constants():
    text = _source("graph.hip")
    out = {}
    for name in ("SMALL_ROWS", "SORT_SERIAL", "SORT_WAVE_CAP", "SORT_LIST", "SORT_PER_THREAD", "SCAN_THREADS"):
        m = re.findall(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, text)
        assert len(m) == 1, "csrc/graph.hip: %d definitions of %s" % (len(m), name)
        out[name] = int(m[0])
    return out


K = _constants()
BLOCK_CAP = K["SCAN_THREADS"] // 64 * K["SORT_WAVE_CAP"]          # SORT_BLOCK_CAP = SORT_WAVES * SORT_WAVE_CAP
BLOCK_MAX = K["SORT_PER_THREAD"] * K["SCAN_THREADS"]


def _form(rows, ncols):
    return "small" if rows <= K["SMALL_ROWS"] and ncols <= K["SMALL_ROWS"] else "multi"


def _transposes():
    """(name, form, list lengths) of every transpose the GPU file builds"""
    out = [(c.name, _form(c.rows, c.ncols), C.list_lengths(C.index_of(c), c.ncols)) for c in C.INDEX_SMALL + C.INDEX_MULTI]
    out += [("dropped_%d" % rows, _form(rows, C.DROPPED_NCOLS), C.list_lengths(C.dropped_index(rows), C.DROPPED_NCOLS))
            for rows in C.DROPPED_ROWS]
    for c in C.PADDED:
        _, col = C.padded_csr_ref(C.padded_of(c))
        out.append(("padded_%d_%d" % (c.rows, c.width), _form(c.rows, c.ncols), C.list_lengths(col, c.ncols)))
    return out


TRANSPOSES = _transposes()


# ------------------------------------------------------------------------------------------ the transposes
def test_the_source_still_has_the_structure_the_tables_assume():
    text = _source("graph.hip")
    assert "SORT_BLOCK_CAP = SORT_WAVES * SORT_WAVE_CAP" in text and "SORT_WAVES = SCAN_THREADS / 64" in text
    assert "rows <= SMALL_ROWS && ncols <= SMALL_ROWS" in text             # the small form of ggpm_csr_transpose
    assert "rows_a > SMALL_ROWS || rows_b > SMALL_ROWS" in text            # the pair's fallback
    assert "slot >= SORT_LIST" in text
    assert BLOCK_MAX == K["SMALL_ROWS"]             # an index of SMALL_ROWS rows and one id fills the workgroup tier exactly


def test_every_index_case_takes_the_form_it_names():
    for c in C.INDEX_SMALL + C.INDEX_MULTI:
        assert _form(c.rows, c.ncols) == c.form, c.name
        assert C.index_of(c).shape == (c.rows,)
        if c.lengths is not None:
            assert tuple(C.list_lengths(C.index_of(c), c.ncols)) == c.lengths
    shapes = {(c.rows, c.ncols) for c in C.INDEX_SMALL + C.INDEX_MULTI}
    assert {(BLOCK_CAP, 1), (BLOCK_CAP + 1, 1), (BLOCK_MAX, 1), (13000, 520)} <= shapes
    assert {(K["SMALL_ROWS"] + 1, 4097), (300, K["SMALL_ROWS"] + 1), (20000, 40)} <= shapes


def test_every_sort_boundary_has_a_list_at_it_and_one_past_it():
    small = set()
    for _, form, lens in TRANSPOSES:
        if form == "small":
            small |= set(int(n) for n in lens)
    for at in (K["SORT_SERIAL"], K["SORT_WAVE_CAP"], BLOCK_CAP):
        assert at in small and at + 1 in small, "no list of %d and %d entries on the small form" % (at, at + 1)
    assert BLOCK_MAX in small                        # (one past it does not fit the small form's rows)
    assert 0 in small and 1 in small


def test_the_overflow_case_has_more_wave_candidates_than_the_table_holds():
    c = next(c for c in C.INDEX_SMALL if c.name == "wave_table_overflow")
    lens = C.list_lengths(C.index_of(c), c.ncols)
    assert int(((lens > K["SORT_SERIAL"]) & (lens <= K["SORT_WAVE_CAP"])).sum()) > K["SORT_LIST"]
    assert _form(c.rows, c.ncols) == "small"
    idx = C.index_of(c)
    assert not np.array_equal(idx, np.sort(idx))                           # shuffled: the lists arrive unsorted
    # shuffled inside the runs of SCAN_THREADS rows that one trip of the workgroup's loops handles: the rows of a list sit in at
    # most two such runs, on many different waves
    assert c.shuffle == "passes" and K["SCAN_THREADS"] == 1024
    for k in (0, 257, c.ncols - 1):
        rows = np.nonzero(idx == k)[0]
        assert len(set(rows // K["SCAN_THREADS"])) <= 2 and len(set(rows % K["SCAN_THREADS"] // 64)) >= 8
    # the workgroup tier's table cannot overflow on the small form (the tables' comment says so instead of faking a case)
    assert (K["SORT_LIST"] + 1) * (K["SORT_WAVE_CAP"] + 1) > K["SMALL_ROWS"]


def test_the_multi_launch_form_has_its_cases_and_only_short_lists():
    multi = [(name, lens) for name, form, lens in TRANSPOSES if form == "multi"]
    assert len([1 for name, _ in multi if not name.startswith("padded")]) >= 3 and len(C.INDEX_MULTI) >= 3
    assert C.MULTI_MAX_LIST <= 512
    for name, lens in multi:
        assert int(lens.max()) <= C.MULTI_MAX_LIST, "%s: a list of %d entries for the serial sort" % (name, lens.max())
    lens = dict(multi)["multi_ncols_16385_mostly_empty"]
    assert (lens == 0).sum() > len(lens) * 0.9
    assert dict(multi)["multi_20000_one_long_column"].max() == C.MULTI_MAX_LIST


def test_the_dropped_id_cases_differ_by_one_valid_row():
    a, b = (C.dropped_index(rows) for rows in C.DROPPED_ROWS)
    assert C.DROPPED_ROWS == (K["SMALL_ROWS"], K["SMALL_ROWS"] + 1)
    assert _form(len(a), C.DROPPED_NCOLS) == "small" and _form(len(b), C.DROPPED_NCOLS) == "multi"
    assert np.array_equal(a, b[:-1]) and 0 <= b[-1] < C.DROPPED_NCOLS
    assert 0.08 < (a == -1).mean() < 0.13
    for bad in (C.DROPPED_NCOLS, C.DROPPED_NCOLS + 5, -7, 2 ** 31 - 1, -2 ** 31):
        assert (a == bad).any()
    valid = (a >= 0) & (a < C.DROPPED_NCOLS)
    rp, cl = C.index_transpose_ref(a, C.DROPPED_NCOLS)
    assert rp[-1] == valid.sum() == len(cl) and not np.isin(np.nonzero(~valid)[0], cl).any()


def test_the_padded_cases_reach_both_forms_of_both_builders():
    rows = sorted({c.rows for c in C.PADDED})
    assert rows[:2] == [K["SMALL_ROWS"], K["SMALL_ROWS"] + 1] and rows[2] > rows[1] and {c.width for c in C.PADDED} == {1, 5}
    assert {_form(c.rows, c.ncols) for c in C.PADDED if c.rows == K["SMALL_ROWS"]} == {"small"}
    for c in C.PADDED:
        p = C.padded_of(c)
        assert p.shape == (c.rows, c.width) and p.min() == 0 and p.max() < c.ncols
        assert (p == 0).all(axis=1).any() and (p != 0).all(axis=1).any()
        assert not (p[0] != 0).any() and (p[-1] != 0).all()                # first row empty, last row (the tail thread) full
        if c.width >= 3:
            assert p[2, 0] != 0 and p[2, 1] == 0 and p[2, 2] != 0          # a zero between two entries
    for a, b in C.PADDED_PAIR:
        assert max(a.rows, b.rows) == K["SMALL_ROWS"] + 1 and min(a.rows, b.rows) < 16


# ------------------------------------------------------------------------------------------ the row movers
def test_segment_sum_conditions_match_the_source():
    text = _source("gather.hip")
    m = re.search(r"const bool vec = (.*?);", text, re.S)
    assert m is not None
    cond = re.sub(r"\s+", " ", m.group(1))
    for term in ("width % 4 == 0", "ld_src % 4 == 0", "ld_out % 4 == 0", "(uintptr_t)src & 15", "(uintptr_t)out & 15"):
        assert term in cond, term
    assert cond.count("&&") == len(C.SEG_CONDITIONS) - 1
    assert "blockIdx.x * 4 + (threadIdx.x >> 6)" in text and "c += 256" in text and "c += 64" in text


def test_every_alignment_condition_is_broken_alone_by_one_case():
    alone = {}
    for c in C.SEGMENT_SUM:
        b = C.seg_broken(c)
        if len(b) == 1 and c.twin:
            alone.setdefault(b[0], []).append(c)
    assert sorted(alone) == sorted(C.SEG_CONDITIONS)
    for name, cases in alone.items():
        for c in cases:
            t = C.seg_case(c.twin)
            assert C.seg_broken(t) == () and (t.rows, t.nsrc, t.seed, t.accumulate, t.lists) == (c.rows, c.nsrc, c.seed, c.accumulate, c.lists)
            assert t.width >= c.width and t.width - c.width < 4
            assert np.array_equal(C.seg_values(t)[0][:, :c.width], C.seg_values(c)[0])
            assert all(np.array_equal(x, y) for x, y in zip(C.seg_lists(t), C.seg_lists(c)))
    assert C.seg_case("break_width").width % 4 and C.seg_case("break_src").src_off == 1 and C.seg_case("break_out").out_off == 1


def test_segment_sum_cases_cover_the_grid_the_loops_and_the_options():
    cases = C.SEGMENT_SUM
    assert {1, 3, 4, 5, 201} <= {c.rows for c in cases}
    assert {1, 3, 4, 64, 252, 256, 260, 300} <= {c.width for c in cases}
    vec = [c for c in cases if not C.seg_broken(c)]
    scalar = [c for c in cases if C.seg_broken(c)]
    assert any(c.width <= 256 for c in vec) and any(c.width > 256 for c in vec)          # one and two trips of 256 columns
    assert any(c.width <= 64 for c in scalar) and any(c.width > 64 for c in scalar)      # one and several trips of 64
    for group in (vec, scalar):
        assert {0, 1} <= {c.accumulate for c in group}
        assert any(c.lists == "long" for c in group)
    assert any(c.zero_to == c.width for c in cases) and any(c.zero_to == c.width + 1 for c in cases)
    assert any(c.zero_to == c.ld_out > c.width + 1 for c in cases) and any(c.zero_to == 0 for c in cases)
    for c in cases + C.SEGMENT_SUM_SPECIAL:
        rowptr, col = C.seg_lists(c)
        lens = np.diff(rowptr)
        assert len(rowptr) == c.rows + 1 and rowptr[-1] == len(col) and (len(col) == 0 or (0 <= col.min() and col.max() < c.nsrc))
        assert c.ld_src >= c.width and c.ld_out >= max(c.width, c.zero_to)
        if c.rows >= 4:
            assert {0, 1, 2, 5} <= set(lens.tolist()) | {5 if c.lists == "long" else -1}
            two = int(np.nonzero(lens == 2)[0][0])
            assert col[rowptr[two]] == col[rowptr[two] + 1]                                # the same source row twice
        if c.lists == "long":
            assert lens.max() == C.LONG_LIST == 9000
    assert len({c.name for c in cases}) == len(cases)


def test_the_special_value_row_is_in_some_lists_and_not_in_others():
    for c in C.SEGMENT_SUM_SPECIAL:
        rowptr, col = C.seg_lists(c)
        k = col[0]
        has = [k in col[rowptr[r]:rowptr[r + 1]] for r in range(c.rows)]
        assert any(has) and not all(has) and sum(has) >= 2
    assert [bool(C.seg_broken(c)) for c in C.SEGMENT_SUM_SPECIAL] == [False, True]


def test_the_other_tables_cover_what_they_name():
    assert {c.rows for c in C.GATHER} == {1, 5, 401} and {c.width for c in C.GATHER} == {1, 63, 64, 65, 300}
    assert {c.col_off for c in C.GATHER} == {0, 5} and {c.zero_to for c in C.GATHER} == {"none", "end", "ld"}
    for c in C.GATHER:
        ld_table, ld_out, zero_to = C.gather_geometry(c)
        idx = C.gather_index(c)
        assert ld_table > c.width and ld_out >= max(zero_to, c.col_off + c.width) and idx.max() < C.GATHER_NTAB
        if c.rows >= 5:
            assert (idx == -1).any() and len(set(idx.tolist())) < c.rows
    assert any(C.gather_index(c)[0] == -1 and C.gather_geometry(c)[2] > c.col_off + c.width for c in C.GATHER)
    assert any(c.rows == 1 and C.gather_index(c)[0] == -1 for c in C.GATHER)
    assert {c.classes for c in C.ONEHOT} == {1, 20, 64, 65, 130} and {c.col_off for c in C.ONEHOT} == {0, 300}
    kinds = set()
    for c in C.ONEHOT:
        ld_out, zero_to = C.onehot_geometry(c)
        end = c.col_off + c.classes
        kinds.add("below" if zero_to < end else "equal" if zero_to == end else "above")
        assert ld_out > max(end, zero_to)
        idx = C.onehot_index(c)
        assert (idx < 0).any() and (idx == c.classes).any() and (idx == c.classes - 1).any()
    assert kinds == {"below", "equal", "above"}
    # the zero fill reaches a workgroup (64 columns) behind the one that holds the last class
    assert any((C.onehot_geometry(c)[1] - 1 - c.col_off) // 64 > (c.classes - 1) // 64 for c in C.ONEHOT)
    names = {c.name: c for c in C.EMBED}
    assert (names["one_row_each"].N1, names["one_row_each"].E1) == (1, 1)
    p = names["product_ld"]
    assert (p.ld_n, p.ld_m) == ((p.atom + 3) // 4 * 4, (p.atom + p.bond + p.pos + 3) // 4 * 4)
    assert names["wide_ld"].ld_n > p.ld_n and names["wide_ld"].ld_m > p.ld_m
    for c in C.EMBED:
        wn, wm = c.atom, c.atom + c.bond + c.pos
        refused = c.ld_n > 256 or c.ld_m > 256 or c.ld_n < wn or c.ld_m < wm           # ggpm_embed_graph's own condition
        assert (c.rc == 3) == refused, c.name
    assert names["message_width_256"].rc == 0 and names["node_width_256"].rc == 0
    assert sum(names["message_width_256"][3:6]) == 256 == names["node_width_256"].atom
    assert sum(names["message_width_257"][3:6]) == 257 == names["node_width_257"].atom
    assert {s for s, _ in C.SUM_SLOTS} == {1, 2, 7} and {n for _, n in C.SUM_SLOTS} == {4, 1024, 1028}
    assert all(n % 4 or n == 0 for n in C.SUM_SLOTS_REFUSED)
    text = _source("mpn_gru.hip")
    assert "float4 acc = ggpm_ldx<B16>(src, 4 * i);" in text and "for (int t = 1; t < slots; ++t) acc = acc +" in text


def test_the_linear_cases_cover_the_three_routes_and_the_options():
    assert {len(c.Ks) for c in C.LINEAR} == {1, 2, 4, 5}
    assert {C.linear_route(c) for c in C.LINEAR} == {"gemm", "ksegments", "chain"}
    assert {c.M for c in C.LINEAR} == {1, 17, 130}
    assert all(set(c.Ks) <= set(C.LINEAR_WIDTHS) for c in C.LINEAR) and {k for c in C.LINEAR for k in c.Ks} == set(C.LINEAR_WIDTHS)
    for route in ("ksegments", "chain"):
        group = [c for c in C.LINEAR if C.linear_route(c) == route]
        assert {c.act for c in group} == {"none", "relu", "tanh"}
        assert {c.bias for c in group} == {True, False} and {c.zero_row0 for c in group} == {True, False}
        assert any(c.ld_out_extra for c in group) and any(c.ld_x_extra for c in group)
        assert any(sum(c.Ks[:i]) % 4 for c in group for i in range(1, len(c.Ks)))         # an unaligned weight slice
    assert C.LINEAR_TOL == 2e-6 and max(sum(c.Ks) for c in C.LINEAR) <= 5000
    assert C.GRADIENT_ROUTES == [("1", "1"), ("0", "1"), ("0", "0")]
    src = open(os.path.join(ROOT, "ggpm_amd", "functional.py")).read()
    assert "if 1 < len(xs) <= 4:" in src                                                   # where linear_route's limits come from


def test_the_wrapper_cases_leave_ids_unused_and_move_fewer_columns_than_the_table_has():
    for c in C.WRAPPERS:
        assert c.width < c.H < c.ld
        idx = C.wrapper_index(c)
        rowptr, col = C.wrapper_lists(c)
        for ids in (idx, col):
            assert 3 not in ids and c.nsrc - 1 not in ids and ids.min() >= 0 and ids.max() < c.nsrc
        assert len(set(idx.tolist())) < len(idx) or c.nsrc > c.rows
        assert (np.diff(rowptr) == 0).any() and len(rowptr) == c.rows + 1
    assert any(len(set(C.wrapper_index(c).tolist())) < c.rows for c in C.WRAPPERS)


# ------------------------------------------------------------------------------------------ the restatements
def test_transpose_ref_against_a_plain_loop():
    rowptr = np.array([0, 2, 2, 5, 6, 8])
    col = np.array([1, 3, 0, 1, 1, -1, 4, 3, 99, 99])              # row 2 names column 1 twice; -1 and 4 (= ncols) are dropped
    want = [[] for _ in range(4)]
    for r in range(5):
        for j in range(rowptr[r], rowptr[r + 1]):
            if 0 <= col[j] < 4:
                want[col[j]].append(r)
    rp, cl = C.transpose_ref(rowptr, col, 5, 4)
    assert rp.tolist() == [0, 1, 4, 4, 6] and cl.tolist() == sum(want, []) == [2, 0, 2, 2, 0, 4]
    idx = np.array([2, 0, 2, -1, 5, 1, 2], dtype=np.int32)
    rp, cl = C.index_transpose_ref(idx, 3)
    assert rp.tolist() == [0, 1, 2, 5] and cl.tolist() == [1, 5, 0, 2, 6]
    assert rp.dtype == np.int32 and cl.dtype == np.int32


def test_padded_csr_ref_against_a_plain_loop():
    p = np.array([[0, 0, 0], [3, 0, 7], [1, 2, 3], [0, 0, 9]], dtype=np.int64)
    rowptr, col = C.padded_csr_ref(p)
    want = [[int(v) for v in row if v != 0] for row in p]
    assert rowptr.tolist() == [0, 0, 2, 5, 6] and col.tolist() == sum(want, []) == [3, 7, 1, 2, 3, 9]


def test_segment_sum_ref_against_a_plain_loop():
    rs = np.random.RandomState(0)
    src = (rs.standard_normal((6, 5)) * np.array([1e-3, 1.0, 1e3, 1e6, 1.0])).astype(np.float32)
    rowptr, col = np.array([0, 3, 3, 4, 9]), np.array([5, 0, 5, 2, 1, 1, 4, 3, 0])
    for accumulate in (0, 1):
        out = np.full((4, 7), -777.25, dtype=np.float32)
        out[:, :3] = rs.standard_normal((4, 3))
        want = out.copy()
        for r in range(4):
            for c in range(3):
                acc = want[r, c] if accumulate else np.float32(0)
                for j in range(rowptr[r], rowptr[r + 1]):
                    acc = np.float32(acc + src[col[j], c])
                want[r, c] = acc
            want[r, 3:6] = 0
        got = C.segment_sum_ref(src, rowptr, col, 3, out, accumulate, 6)
        assert got is out and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[:, 6] == -777.25).all() and (got[1, :3] == (want[1, :3] if accumulate else 0)).all()
    # the order matters to the bits: that is what makes the comparison a test of the kernel's order
    big = np.array([[1e8], [1.0], [-1e8]], dtype=np.float32)
    a = C.segment_sum_ref(big, [0, 3], [0, 1, 2], 1, np.zeros((1, 1), np.float32), 0, 0)
    b = C.segment_sum_ref(big, [0, 3], [0, 2, 1], 1, np.zeros((1, 1), np.float32), 0, 0)
    assert a[0, 0] == 0.0 and b[0, 0] == 1.0


def test_the_backward_restatement_is_the_gradient_of_the_forward():
    """segment_sum_ref over transpose_ref's lists against fp64 autograd of the forward, within the bound of an fp32 chain"""
    c = C.WRAPPERS[0]
    rowptr, col = C.wrapper_lists(c)
    rs = np.random.RandomState(1)
    g = rs.standard_normal((c.rows, c.width)).astype(np.float32)
    rpT, clT = C.transpose_ref(rowptr, col, c.rows, c.nsrc)
    got = C.segment_sum_ref(g, rpT, clT, c.width, np.full((c.nsrc, c.width), 7.0, np.float32), 0, 0)
    src = torch.zeros(c.nsrc, c.width, dtype=torch.float64, requires_grad=True)
    row_of = np.repeat(np.arange(c.rows), np.diff(rowptr))
    out = torch.zeros(c.rows, c.width, dtype=torch.float64).index_add(0, torch.from_numpy(row_of), src[torch.from_numpy(col).long()])
    out.backward(torch.from_numpy(g).double())
    n = np.diff(rpT).max()
    bound = (n - 1) * 2.0 ** -24 * np.abs(g).max() * n + 1e-30
    assert np.abs(got - src.grad.numpy()).max() <= bound
    assert (got[3] == 0).all() and (got[c.nsrc - 1] == 0).all()


def test_gather_onehot_embed_and_sum_slots_refs_against_plain_constructions():
    table = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    out = C.gather_rows_ref(table, [2, -1, 2, 0], 2, np.full((4, 7), 7.0, np.float32), 1, 5)
    assert out.tolist() == [[7, 7, 8, 0, 0, 7, 7], [7, 0, 0, 0, 0, 7, 7], [7, 7, 8, 0, 0, 7, 7], [7, 1, 2, 0, 0, 7, 7]]
    out = C.gather_rows_ref(table, [3], 3, np.full((1, 5), 7.0, np.float32), 0, 0)
    assert out.tolist() == [[10, 11, 12, 7, 7]]
    out = C.onehot_ref([1, -1, 3, 2], 3, np.full((4, 7), 7.0, np.float32), 2, 6)
    assert out.tolist() == [[7, 7, 0, 1, 0, 0, 7], [7, 7, 0, 0, 0, 0, 7], [7, 7, 0, 0, 0, 0, 7], [7, 7, 0, 0, 1, 0, 7]]
    out = C.onehot_ref([0], 2, np.full((1, 4), 7.0, np.float32), 1, 1)
    assert out.tolist() == [[7, 1, 0, 7]]
    c = C.EMBED[1]
    fnode, fmess = C.embed_inputs(c)
    hnode, hmess = C.embed_graph_ref(fnode, fmess, c.atom, c.bond, c.pos, c.ld_n, c.ld_m)

    def eye(ids, n):
        e = np.vstack([np.eye(n, dtype=np.float32), np.zeros((1, n), np.float32)])       # row n: all zero, for ids out of range
        return e[np.where((ids >= 0) & (ids < n), ids, n)]

    assert np.array_equal(hnode[:, :c.atom], eye(fnode, c.atom)) and (hnode[:, c.atom:] == 0).all()
    want = np.hstack([eye(fnode[fmess[:, 0]], c.atom), eye(fmess[:, 2], c.bond), eye(fmess[:, 3], c.pos)])
    assert np.array_equal(hmess[:, :want.shape[1]], want) and (hmess[:, want.shape[1]:] == 0).all()
    assert (hnode[1] == 0).all() and (hnode[2] == 0).all() and hnode[3, c.atom - 1] == 1
    assert (hmess[3, c.atom:c.atom + c.bond] == 0).all() and (hmess[7, c.atom + c.bond:] == 0).all()
    src = np.array([[1e8, 1.0], [1.0, 2.0], [-1e8, 3.0]], dtype=np.float32)
    assert C.sum_slots_ref(src).tolist() == [0.0, 6.0] and C.sum_slots_ref(src[:1]).tolist() == [1e8, 1.0]
