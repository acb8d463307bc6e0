"""GPU: the CSR builders of csrc/graph.hip, the row movers of csrc/gather.hip, ggpm_sum_slots and the autograd wrappers over
them, on every path they take, against the host restatements of tests/row_op_cases.py.

Parts 1 and 2 are exact.  The builders are integer work: `rowptr` and `col[:rowptr[-1]]` must equal the restatement.  The row
movers copy, or add fp32 values one after the other in an order the restatement repeats, so the whole output ALLOCATION --
guard rows before and after, the columns between the written block and the leading dimension -- is compared bit for bit
with what the restatement makes of the same sentinel-filled buffer: a write outside the contract shows like a wrong value.
Sources sit in NaN-filled allocations (NaN in every pad column and guard row), so a read outside the contract shows too.
Part 3 compares the index wrappers of functional.py exactly and `linear` against fp64 under the GEMM bar (LINEAR_TOL).
tests/test_row_op_cases_cpu.py holds the tables to the constants of the source."""

import numpy as np
import pytest
import torch

import row_op_cases as C
from golden_utils import rel_err
from ggpm_amd import _lib
from ggpm_amd import functional as F_

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL, GUARD = -777.25, -12345, 64
OK, ERR_ARG, ERR_UNSUPPORTED = _lib.GGPM_OK, _lib.GGPM_ERR_ARG, _lib.GGPM_ERR_UNSUPPORTED


def _dev():
    return torch.device("cuda:0")


def _s():
    return F_._stream()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _ints(n):
    """n int32 inside a sentinel-filled allocation with GUARD words before and after -> (allocation, view)"""
    buf = torch.full((n + 2 * GUARD,), ISENTINEL, dtype=torch.int32, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == ISENTINEL).all() and (b[-GUARD:] == ISENTINEL).all())


def _floats(rows, ld, off, fill, values=None):
    """[rows, ld] view `off` floats into a 16-byte aligned allocation filled with `fill`, four guard rows before and after;
    `values` go to its first columns -> (allocation, view, (start, stop) of the view inside the flat allocation)"""
    buf = torch.full(((rows + 8) * ld + 8,), fill, dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    lo = 4 * ld + off
    view = buf[lo:lo + rows * ld].view(rows, ld)
    if values is not None:
        view[:, :values.shape[1]] = _t(values)
    return buf, view, (lo, lo + rows * ld)


def _host(buf, span, rows, ld):
    """host copy of an allocation and the writable [rows, ld] view of it where the device view sits"""
    flat = buf.cpu().numpy().copy()
    return flat, flat[span[0]:span[1]].reshape(rows, ld)


# ============================================================================================== 1. CSR builders
def _transpose_raw(rowptr, col, rows, ncols):
    """ggpm_csr_transpose on guarded buffers -> (rowptrT, colT[:capacity]); the guards and the unused tail of colT are checked"""
    nnz = int(rowptr[-1])
    rp, cl = _t(np.asarray(rowptr, dtype=np.int32)), _t(np.asarray(col, dtype=np.int32))
    (b0, rpT), (b1, clT), (b2, cur) = _ints(ncols + 1), _ints(nnz), _ints(ncols)
    rc = _lib.load().ggpm_csr_transpose(F_._p(rp), F_._p(cl), rows, ncols, F_._p(rpT), F_._p(clT), F_._p(cur), _s())
    assert rc == OK
    torch.cuda.synchronize()
    assert _guards_intact(b0) and _guards_intact(b1) and _guards_intact(b2)
    rpT, clT = rpT.cpu().numpy(), clT.cpu().numpy()
    assert (clT[rpT[-1]:] == ISENTINEL).all()                  # nothing written past the in-range entries
    return rpT, clT


def _index_T(idx, ncols):
    """csr_from_index(idx).T, as the backward passes build it -> (rowptrT, colT)"""
    T = F_.csr_from_index(_t(idx), ncols=ncols).T
    assert (T.rows, T.ncols) == (ncols, len(idx))
    return T.rowptr.cpu().numpy(), T.col.cpu().numpy()


def _assert_transpose(rpT, clT, want):
    assert np.array_equal(rpT, want[0])
    assert np.array_equal(clT[:rpT[-1]], want[1])


@pytest.mark.parametrize("c", C.INDEX_SMALL + C.INDEX_MULTI, ids=lambda c: c.name)
def test_transpose_of_an_index_on_every_sort_tier_and_form(c):
    """csr_from_index(idx).T and the raw entry point: lists exactly at and past SORT_SERIAL, SORT_WAVE_CAP and SORT_BLOCK_CAP,
    a full 16 384-entry list, more wave-tier lists than the candidate table holds (the surplus is sorted serially), and the
    multi-launch form through rows, through ncols alone (most columns empty) and at 20 000 rows."""
    idx = C.index_of(c)
    want = C.index_transpose_ref(idx, c.ncols)
    assert want[0][-1] == c.rows
    _assert_transpose(*_index_T(idx, c.ncols), want)
    _assert_transpose(*_transpose_raw(np.arange(c.rows + 1), idx, c.rows, c.ncols), want)


def test_both_transpose_forms_drop_the_same_ids():
    """-1 in a tenth of the rows, ids at and past ncols, INT_MIN and INT_MAX: absent from both forms' lists, rowptr[-1] the
    number of in-range entries, and the lists of the 16 384 shared rows identical (16 385 rows = the same index plus one
    valid row, on the multi-launch form)."""
    ncols, lists = C.DROPPED_NCOLS, []
    for rows in C.DROPPED_ROWS:
        idx = C.dropped_index(rows)
        want = C.index_transpose_ref(idx, ncols)
        valid = (idx >= 0) & (idx < ncols)
        for rpT, clT in (_transpose_raw(np.arange(rows + 1), idx, rows, ncols), _index_T(idx, ncols)):
            _assert_transpose(rpT, clT, want)
            assert rpT[-1] == valid.sum()
            assert not np.isin(np.nonzero(~valid)[0], clT[:rpT[-1]]).any()
        lists.append([clT[rpT[k]:rpT[k + 1]] for k in range(ncols)])
    shared = C.DROPPED_ROWS[0]
    for k in range(ncols):
        assert np.array_equal(lists[0][k], lists[1][k][lists[1][k] < shared])
    assert sum(len(x) for x in lists[1]) == sum(len(x) for x in lists[0]) + 1
    assert lists[1][C.DROPPED_EXTRA_ID][-1] == shared


def _padded_raw(padded):
    rows, width = padded.shape
    (b0, rp), (b1, cl) = _ints(rows + 1), _ints(rows * width)
    dev = _t(padded)
    rc = _lib.load().ggpm_padded_to_csr(F_._p(dev), rows, width, F_._p(rp), F_._p(cl), _s())
    assert rc == OK
    torch.cuda.synchronize()
    assert _guards_intact(b0) and _guards_intact(b1)
    rp, cl = rp.cpu().numpy(), cl.cpu().numpy()
    assert (cl[rp[-1]:] == ISENTINEL).all()
    return rp, cl


@pytest.mark.parametrize("c", C.PADDED, ids=lambda c: "%dx%d" % (c.rows, c.width))
def test_csr_from_padded_and_its_transpose_at_and_past_the_single_workgroup_limit(c):
    """16 384 rows (one workgroup), 16 385 and 20 000 (count_nonzero_rows, the in-place scan, fill_csr_from_padded) at widths 1
    and 5: rows of zeros, full rows, a zero between two entries.  The transposes take the small form at 16 384 rows and the
    multi-launch form beyond."""
    padded = C.padded_of(c)
    want = C.padded_csr_ref(padded)
    csr = F_.csr_from_padded(_t(padded), ncols=c.ncols)
    for rp, cl in ((csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()), _padded_raw(padded)):
        assert np.array_equal(rp, want[0]) and np.array_equal(cl[:rp[-1]], want[1])
    wantT = C.transpose_ref(want[0], want[1], c.rows, c.ncols)
    T = csr.T
    _assert_transpose(T.rowptr.cpu().numpy(), T.col.cpu().numpy(), wantT)
    _assert_transpose(*_transpose_raw(want[0], want[1], c.rows, c.ncols), wantT)


@pytest.mark.parametrize("pair", C.PADDED_PAIR, ids=["large_small", "small_large"])
def test_padded_to_csr_pair_falls_back_to_two_calls_past_the_limit(pair):
    lib = _lib.load()
    pads = [C.padded_of(c) for c in pair]
    dev = [_t(p) for p in pads]
    outs = [(_ints(c.rows + 1), _ints(c.rows * c.width)) for c in pair]
    (a, b), ((ra, ca), (rb, cb)) = pair, [(o[0][1], o[1][1]) for o in outs]
    rc = lib.ggpm_padded_to_csr_pair(F_._p(dev[0]), a.rows, a.width, F_._p(ra), F_._p(ca),
                                     F_._p(dev[1]), b.rows, b.width, F_._p(rb), F_._p(cb), _s())
    assert rc == OK
    torch.cuda.synchronize()
    for p, ((b0, rp), (b1, cl)) in zip(pads, outs):
        assert _guards_intact(b0) and _guards_intact(b1)
        want = C.padded_csr_ref(p)
        one = _padded_raw(p)                                      # the separate call
        rp, cl = rp.cpu().numpy(), cl.cpu().numpy()
        assert np.array_equal(rp, want[0]) and np.array_equal(cl[:rp[-1]], want[1]) and (cl[rp[-1]:] == ISENTINEL).all()
        assert np.array_equal(rp, one[0]) and np.array_equal(cl, one[1])


def _refused(call, args, bad, outputs, code=ERR_ARG):
    """`call(*args)` with each replacement of `bad` ({position: value}) must return `code` and leave `outputs` unchanged"""
    before = [o.cpu().numpy().copy() for o in outputs]
    for changes in bad:
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        assert call(*a) == code, changes
    torch.cuda.synchronize()
    for o, b in zip(outputs, before):
        assert np.array_equal(o.cpu().numpy().view(np.uint8), b.view(np.uint8))


def test_the_builders_refuse_null_pointers_and_empty_shapes():
    lib = _lib.load()
    padded = _t(np.array([[1, 0], [2, 3], [0, 0]], dtype=np.int64))
    (b0, rp), (b1, cl), (b2, cur) = _ints(4), _ints(6), _ints(5)
    p = lambda t: t.data_ptr()
    args = [p(padded), 3, 2, p(rp), p(cl), _s()]
    _refused(lib.ggpm_padded_to_csr, args, [{0: None}, {3: None}, {4: None}, {1: 0}, {1: -1}, {2: 0}, {2: -3}], [b0, b1])
    pair = args[:5] + args
    _refused(lib.ggpm_padded_to_csr_pair, pair, [{k: None} for k in (0, 3, 4, 5, 8, 9)] + [{k: 0} for k in (1, 2, 6, 7)]
             + [{1: -1}, {7: -2}, {1: 20000, 8: None}], [b0, b1])
    rowptr, col = _t(np.array([0, 1, 2, 3], dtype=np.int32)), _t(np.array([1, 0, 4], dtype=np.int32))
    (b3, rpT), (b4, clT) = _ints(6), _ints(3)
    targs = [p(rowptr), p(col), 3, 5, p(rpT), p(clT), p(cur), _s()]
    _refused(lib.ggpm_csr_transpose, targs, [{k: None} for k in (0, 1, 4, 5, 6)] + [{2: 0}, {2: -1}, {3: 0}, {3: -1},
                                                                                   {2: 20000, 4: None}, {3: 20000, 6: None}],
             [b2, b3, b4])
    assert lib.ggpm_padded_to_csr(*args) == OK and lib.ggpm_csr_transpose(*targs) == OK      # the unchanged calls are accepted
    torch.cuda.synchronize()
    assert rp.cpu().tolist() == [0, 1, 3, 3] and rpT.cpu().tolist() == [0, 1, 2, 2, 2, 3]


# ============================================================================================== 2. row movers
def _segment_sum(c, special_row=None):
    """run one SegCase -> (got allocation, wanted allocation, [rows, ld_out] views of both, the source values)"""
    src_v, old = C.seg_values(c)
    if special_row is not None:
        src_v[special_row, C.SEG_SPECIAL_COLUMNS[0]] = np.nan
        src_v[special_row, C.SEG_SPECIAL_COLUMNS[1]] = np.inf
    rowptr, col = C.seg_lists(c)
    _, s, _ = _floats(c.nsrc, c.ld_src, c.src_off, float("nan"), src_v)
    obuf, o, span = _floats(c.rows, c.ld_out, c.out_off, SENTINEL, old if c.accumulate else None)
    assert (s.data_ptr() % 16 == 0) == (c.src_off % 4 == 0) and (o.data_ptr() % 16 == 0) == (c.out_off % 4 == 0)
    want, want_view = _host(obuf, span, c.rows, c.ld_out)
    C.segment_sum_ref(src_v, rowptr, col, c.width, want_view, c.accumulate, c.zero_to)
    rp, cl = _t(rowptr), _t(col)
    rc = _lib.load().ggpm_segment_sum(F_._p(s), c.ld_src, F_._p(rp), F_._p(cl), c.rows, c.width, F_._p(o), c.ld_out,
                                      c.accumulate, c.zero_to, _s())
    assert rc == OK
    got, got_view = _host(obuf, span, c.rows, c.ld_out)
    return got, want, got_view, want_view, src_v


@pytest.mark.parametrize("c", C.SEGMENT_SUM, ids=lambda c: c.name)
def test_segment_sum_bits_on_both_kernels(c):
    """ggpm_segment_sum against the sequential float32 accumulation in list order (from 0, or from what `out` held): the same
    bits, in the 16-byte kernel and in the scalar one.  Rows 1 .. 201 (the tail of the four-rows-per-workgroup grid), widths on
    both sides of a trip of either column loop, empty / single / repeated / 9 000-entry lists, accumulate, every zero_to.
    A case that fails ONE alignment condition must also repeat its aligned twin's columns bit for bit."""
    got, want, got_view, _, _ = _segment_sum(c)
    assert _same_bits(got, want)
    if c.twin:
        t = C.seg_case(c.twin)
        assert C.seg_broken(c) and not C.seg_broken(t)
        _, _, twin_view, _, _ = _segment_sum(t)
        assert _same_bits(got_view[:, :c.width], twin_view[:, :c.width])


@pytest.mark.parametrize("c", C.SEGMENT_SUM_SPECIAL, ids=lambda c: c.name)
def test_segment_sum_carries_nan_and_inf_to_the_rows_that_list_them(c):
    rowptr, col = C.seg_lists(c)
    k = int(col[0])
    got, want, got_view, want_view, _ = _segment_sum(c, special_row=k)
    lists_k = np.array([k in col[rowptr[r]:rowptr[r + 1]] for r in range(c.rows)])
    nan_col, inf_col = C.SEG_SPECIAL_COLUMNS
    assert np.array_equal(np.isnan(got_view[:, nan_col]), lists_k) and np.array_equal(np.isposinf(got_view[:, inf_col]), lists_k)
    special = np.zeros_like(got_view, dtype=bool)
    special[lists_k, nan_col] = special[lists_k, inf_col] = True
    assert np.isfinite(got_view[~special]).all()
    finite = ~np.isnan(want)                                       # (a NaN's payload is not part of the contract)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(got[finite], want[finite])


@pytest.mark.parametrize("c", C.GATHER, ids=lambda c: "r%d_w%d_off%d_%s" % c[:4])
def test_gather_rows_with_column_offset_fill_and_negative_ids(c):
    """numpy indexing; ld_table > width with NaN behind every table row; a -1 gives a zero row AND still gets its zero_to fill"""
    ld_table, ld_out, zero_to = C.gather_geometry(c)
    table = np.random.RandomState(c.rows * 7 + c.width).standard_normal((C.GATHER_NTAB, c.width)).astype(np.float32)
    idx = C.gather_index(c)
    _, t, _ = _floats(C.GATHER_NTAB, ld_table, 0, float("nan"), table)
    obuf, o, span = _floats(c.rows, ld_out, 0, SENTINEL)
    want, want_view = _host(obuf, span, c.rows, ld_out)
    C.gather_rows_ref(table, idx, c.width, want_view, c.col_off, zero_to)
    ids = _t(idx)
    rc = _lib.load().ggpm_gather_rows(F_._p(t), ld_table, F_._p(ids), c.rows, c.width, F_._p(o), ld_out, c.col_off, zero_to, _s())
    assert rc == OK
    got, got_view = _host(obuf, span, c.rows, ld_out)
    assert _same_bits(got, want)
    neg = idx < 0
    if neg.any():
        assert (got_view[neg, c.col_off:max(zero_to, c.col_off + c.width)] == 0).all()
        assert (got_view[neg, :c.col_off] == SENTINEL).all()


@pytest.mark.parametrize("c", C.ONEHOT, ids=lambda c: "k%d_off%d_zero%s" % c)
def test_onehot_span_fill_and_ids_out_of_range(c):
    """an id below 0 or >= classes gives an all-zero span; the columns left of col_off and right of the span keep their bits"""
    ld_out, zero_to = C.onehot_geometry(c)
    idx = C.onehot_index(c)
    rows = len(idx)
    obuf, o, span = _floats(rows, ld_out, 0, SENTINEL)
    want, want_view = _host(obuf, span, rows, ld_out)
    C.onehot_ref(idx, c.classes, want_view, c.col_off, zero_to)
    ids = _t(idx)
    assert _lib.load().ggpm_onehot(F_._p(ids), rows, c.classes, F_._p(o), ld_out, c.col_off, zero_to, _s()) == OK
    got, got_view = _host(obuf, span, rows, ld_out)
    assert _same_bits(got, want)
    out_of_range = (idx < 0) | (idx >= c.classes)
    assert (got_view[out_of_range, c.col_off:c.col_off + c.classes] == 0).all()
    assert (got_view[~out_of_range, c.col_off:c.col_off + c.classes].sum(axis=1) == 1).all()


@pytest.mark.parametrize("c", C.EMBED, ids=lambda c: c.name)
def test_embed_graph_blocks_pads_limits_and_values_out_of_range(c):
    """[onehot(atom of the source) | onehot(bond type f[2]) | onehot(position f[3])], pad columns up to ld zero, a value outside
    its range a zero block; widths of exactly 256 accepted, 257 (or ld below the width) refused with nothing written"""
    fnode, fmess = C.embed_inputs(c)
    nbuf, hn, nspan = _floats(c.N1, c.ld_n, 0, SENTINEL)
    mbuf, hm, mspan = _floats(c.E1, c.ld_m, 0, SENTINEL)
    want_n, want_nv = _host(nbuf, nspan, c.N1, c.ld_n)
    want_m, want_mv = _host(mbuf, mspan, c.E1, c.ld_m)
    fn, fm = _t(fnode), _t(fmess)
    rc = _lib.load().ggpm_embed_graph(F_._p(fn), c.N1, F_._p(fm), c.E1, c.atom, c.bond, c.pos, F_._p(hn), c.ld_n, F_._p(hm),
                                      c.ld_m, _s())
    assert rc == c.rc
    if rc == OK:
        want_nv[:], want_mv[:] = C.embed_graph_ref(fnode, fmess, c.atom, c.bond, c.pos, c.ld_n, c.ld_m)
    assert _same_bits(nbuf.cpu().numpy(), want_n) and _same_bits(mbuf.cpu().numpy(), want_m)
    if c.name == "product_ld":                                     # functional.embed_graph chooses these leading dimensions
        hnode, hmess = F_.embed_graph(_t(fnode), _t(fmess), c.atom, c.bond, c.pos)
        assert hnode.shape == want_nv.shape and hmess.shape == want_mv.shape
        assert _same_bits(hnode.cpu().numpy(), want_nv) and _same_bits(hmess.cpu().numpy(), want_mv)


@pytest.mark.parametrize("slots,n", C.SUM_SLOTS)
def test_sum_slots_bits(slots, n):
    """sum_slots_k starts from slot 0 and adds the slots upwards: the same bits as that float32 chain"""
    rs = np.random.RandomState(slots * 10000 + n)
    src = (rs.standard_normal((slots, n)) * np.exp(rs.uniform(-8, 8, size=(slots, 1)))).astype(np.float32)
    _, s, _ = _floats(slots, n, 0, float("nan"), src)
    obuf, o, span = _floats(1, n, 0, SENTINEL)
    want, want_view = _host(obuf, span, 1, n)
    want_view[0] = C.sum_slots_ref(src)
    assert _lib.load().ggpm_sum_slots(F_._p(s), slots, n, F_._p(o), _s()) == OK
    assert _same_bits(obuf.cpu().numpy(), want)


def test_the_row_movers_refuse_what_their_entry_points_check():
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    src = torch.ones(4, 8, device=_dev())
    rowptr, col, idx = (_t(np.array(a, dtype=np.int32)) for a in ([0, 1, 2], [1, 0], [1, 0]))
    obuf, o, _ = _floats(2, 8, 0, SENTINEL)
    none = lambda ks: [{k: None} for k in ks]
    _refused(lib.ggpm_segment_sum, [p(src), 8, p(rowptr), p(col), 2, 4, p(o), 8, 0, 8, _s()],
             none((0, 2, 3, 6)) + [{4: 0}, {4: -1}, {5: 0}, {5: -4}], [obuf])
    _refused(lib.ggpm_gather_rows, [p(src), 8, p(idx), 2, 4, p(o), 8, 0, 8, _s()],
             none((0, 2, 5)) + [{3: 0}, {3: -1}, {4: 0}, {4: -4}], [obuf])
    _refused(lib.ggpm_onehot, [p(idx), 2, 4, p(o), 8, 0, 8, _s()], none((0, 3)) + [{1: 0}, {1: -1}, {2: 0}, {2: -4}], [obuf])
    fnode, fmess = _t(np.array([1, 0], dtype=np.int64)), _t(np.array([[0, 1, 0, 0], [1, 0, 1, 1]], dtype=np.int64))
    mbuf, m, _ = _floats(2, 8, 0, SENTINEL)
    _refused(lib.ggpm_embed_graph, [p(fnode), 2, p(fmess), 2, 3, 2, 2, p(o), 8, p(m), 8, _s()],
             none((0, 2, 7, 9)) + [{1: 0}, {1: -1}, {3: 0}, {3: -1}], [obuf, mbuf])
    _refused(lib.ggpm_sum_slots, [p(src), 2, 8, p(o), _s()],
             none((0, 3)) + [{1: 0}, {1: -1}] + [{2: n} for n in C.SUM_SLOTS_REFUSED], [obuf])
    assert lib.ggpm_segment_sum(p(src), 8, p(rowptr), p(col), 2, 4, p(o), 8, 0, 8, _s()) == OK       # the unchanged call
    assert (o.cpu().numpy() == np.array([[1] * 4 + [0] * 4] * 2, dtype=np.float32)).all()


# ============================================================================================== 3. autograd wrappers
def _table_view(c, values):
    """the [nsrc, H] leaf that views a NaN-filled [nsrc + 2, ld] buffer from its second row on"""
    base = torch.full((c.nsrc + 2, c.ld), float("nan"), dtype=torch.float32, device=_dev())
    base[1:c.nsrc + 1, :c.H] = _t(values)
    return base[1:c.nsrc + 1, :c.H].requires_grad_()


def _wrapper_values(c, cols_out):
    rs = np.random.RandomState(c.seed + 7)
    return rs.standard_normal((c.nsrc, c.H)).astype(np.float32), rs.standard_normal((c.rows, cols_out)).astype(np.float32)


def _backward_ref(g, rowptr, col, c):
    """the gradient of a [nsrc, H] table whose first `width` columns were gathered by the lists: every transposed list applied
    in ascending row order, the remaining columns zero"""
    rpT, clT = C.transpose_ref(rowptr, col, c.rows, c.nsrc)
    return C.segment_sum_ref(g, rpT, clT, c.width, np.full((c.nsrc, c.H), SENTINEL, dtype=np.float32), 0, c.H)


def _set_route(monkeypatch, route):
    monkeypatch.setenv("GGPM_DEFER_WGRADS", route[0])
    monkeypatch.setenv("GGPM_SIDE_STREAM", route[1])


@pytest.mark.parametrize("c", C.WRAPPERS, ids=lambda c: "r%d_n%d_w%d" % (c.rows, c.nsrc, c.width))
def test_segment_sum_wrapper_forward_and_backward_bits(c):
    vals, g = _wrapper_values(c, c.ld)
    rowptr, col = C.wrapper_lists(c)
    src = _table_view(c, vals)
    csr = F_.CSR(_t(rowptr), _t(col), c.rows, c.nsrc)
    out = F_.segment_sum(src, csr, c.width)
    want = C.segment_sum_ref(vals, rowptr, col, c.width, np.full((c.rows, c.ld), SENTINEL, dtype=np.float32), 0, c.ld)
    assert out.shape == want.shape and _same_bits(out.detach().cpu().numpy(), want)
    out.backward(_t(g))
    torch.cuda.synchronize()
    grad = src.grad.cpu().numpy()
    assert grad.shape == (c.nsrc, c.H) and _same_bits(grad, _backward_ref(g, rowptr, col, c))
    assert (grad[3] == 0).all() and (grad[c.nsrc - 1] == 0).all() and (grad[:, c.width:] == 0).all()


@pytest.mark.parametrize("route", C.GRADIENT_ROUTES, ids=C.GRADIENT_ROUTE_IDS)
@pytest.mark.parametrize("c", C.WRAPPERS, ids=lambda c: "r%d_n%d_w%d" % (c.rows, c.nsrc, c.width))
def test_gather_rows_wrapper_forward_and_backward_bits(c, route, monkeypatch):
    """the table's gradient through the deferred end-of-pass scatter and through the node itself: the same bits"""
    _set_route(monkeypatch, route)
    ld_out = (c.width + 3) // 4 * 4 + 4
    vals, g = _wrapper_values(c, ld_out)
    idx = C.wrapper_index(c)
    table = _table_view(c, vals)
    idx_d = _t(idx)
    out = F_.gather_rows(table, idx_d, F_.csr_from_index(idx_d, ncols=c.nsrc), c.width, ld_out)
    want = C.gather_rows_ref(vals, idx, c.width, np.full((c.rows, ld_out), SENTINEL, dtype=np.float32), 0, ld_out)
    assert out.shape == want.shape and _same_bits(out.detach().cpu().numpy(), want)
    out.backward(_t(g))
    torch.cuda.synchronize()
    grad = table.grad.cpu().numpy()
    assert grad.shape == (c.nsrc, c.H) and _same_bits(grad, _backward_ref(g, np.arange(c.rows + 1), idx, c))
    assert (grad[3] == 0).all() and (grad[c.nsrc - 1] == 0).all()


@pytest.mark.parametrize("c", C.WRAPPERS, ids=lambda c: "r%d_n%d_w%d" % (c.rows, c.nsrc, c.width))
def test_tree_message_input_wrapper_forward_and_backward_bits(c):
    """[hnode[src, :width] | onehot(pos)] with the pad zeroed; positions below 0 and past the last give zero blocks"""
    n_pos = C.TREE_POSITIONS
    ld_out = (c.width + n_pos + 3) // 4 * 4 + 4
    vals, g = _wrapper_values(c, ld_out)
    idx = C.wrapper_index(c)
    pos = np.random.RandomState(c.seed + 9).randint(-1, n_pos + 1, size=c.rows).astype(np.int32)
    pos[:3] = (-1, n_pos, n_pos - 1)
    hnode = _table_view(c, vals)
    idx_d = _t(idx)
    out = F_.tree_message_input(hnode, idx_d, F_.csr_from_index(idx_d, ncols=c.nsrc), _t(pos), c.width, n_pos, ld_out)
    want = C.gather_rows_ref(vals, idx, c.width, np.full((c.rows, ld_out), SENTINEL, dtype=np.float32), 0, 0)
    want = C.onehot_ref(pos, n_pos, want, c.width, ld_out)
    assert not (want == SENTINEL).any() and _same_bits(out.detach().cpu().numpy(), want)
    out.backward(_t(g))
    torch.cuda.synchronize()
    grad = hnode.grad.cpu().numpy()
    assert grad.shape == (c.nsrc, c.H) and _same_bits(grad, _backward_ref(g, np.arange(c.rows + 1), idx, c))
    assert (grad[3] == 0).all() and (grad[c.nsrc - 1] == 0).all()


_ACT = {"none": F_.ACT_NONE, "relu": F_.ACT_RELU, "tanh": F_.ACT_TANH}


def _linear_inputs(c, xs):
    """every input as a [M, K] leaf inside a NaN-filled [M, K + ld_x_extra] buffer"""
    out = []
    for x in xs:
        buf = torch.full((c.M, x.shape[1] + c.ld_x_extra), float("nan"), dtype=torch.float32, device=_dev())
        buf[:, :x.shape[1]] = _t(x)
        out.append(buf[:, :x.shape[1]].requires_grad_())
    return out


def _linear_fp64(c, xs, W, b, g):
    """the same computation in fp64 torch on the CPU -> (y, [dx], dW, db)"""
    xd = [torch.from_numpy(x).double().requires_grad_() for x in xs]
    Wd = torch.from_numpy(W).double().requires_grad_()
    bd = torch.from_numpy(b).double().requires_grad_()
    pre = torch.cat(xd, dim=1) @ Wd.t() + (bd if c.bias else 0)
    y = {"none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh}[c.act](pre)
    if c.zero_row0:
        mask = torch.ones(c.M, 1, dtype=torch.float64)
        mask[0] = 0
        y = y * mask
    (y * torch.from_numpy(g).double()).sum().backward()
    return y.detach().numpy(), [x.grad.numpy() for x in xd], Wd.grad.numpy(), bd.grad.numpy() if c.bias else None


@pytest.mark.parametrize("route", C.GRADIENT_ROUTES, ids=C.GRADIENT_ROUTE_IDS)
@pytest.mark.parametrize("c", C.LINEAR, ids=lambda c: c.name)
def test_linear_on_its_three_forward_routes_against_fp64(c, route, monkeypatch):
    """One GEMM, gemm_ksegments (2 .. 4 inputs) and the accumulate chain (5 inputs), each under the three gradient routes:
    y, every dx, dW and db against fp64 under the bar test_gemm_against_fp64 holds a product of K <= 5000 to; the pad columns of
    y exactly zero; inputs whose pad columns hold NaN."""
    _set_route(monkeypatch, route)
    xs, W, b, g = C.linear_values(c)
    y_ref, dx_ref, dW_ref, db_ref = _linear_fp64(c, xs, W, b, g)
    weight = torch.nn.Parameter(_t(W))
    bias = torch.nn.Parameter(_t(b)) if c.bias else None
    xd = _linear_inputs(c, xs)
    ld_out = F_.padded_hidden(c.N) + c.ld_out_extra
    y = F_.linear(xd, c.Ks, weight, bias, act=_ACT[c.act], zero_row0=c.zero_row0, ld_out=ld_out)
    got = y.detach().cpu().numpy()
    assert got.shape == (c.M, ld_out) and (got[:, c.N:] == 0).all()
    assert rel_err(got[:, :c.N], y_ref) < C.LINEAR_TOL
    G = np.random.RandomState(3).standard_normal((c.M, ld_out)).astype(np.float32)      # the pad columns' gradient is ignored
    G[:, :c.N] = g
    y.backward(_t(G))
    torch.cuda.synchronize()
    for i, (x, ref) in enumerate(zip(xd, dx_ref)):
        assert x.grad.shape == ref.shape and rel_err(x.grad.cpu().numpy(), ref) < C.LINEAR_TOL, "dx of segment %d" % i
    assert rel_err(weight.grad.cpu().numpy(), dW_ref) < C.LINEAR_TOL
    if c.bias:
        assert rel_err(bias.grad.cpu().numpy(), db_ref) < C.LINEAR_TOL


@pytest.mark.parametrize("c", [c for c in C.LINEAR if C.linear_route(c) == "chain"], ids=lambda c: c.name)
def test_the_five_segment_chain_equals_four_segments_of_the_same_input(c):
    xs, W, b, _ = C.linear_values(c)
    weight, bias = _t(W), _t(b) if c.bias else None
    merged = xs[:3] + [np.concatenate(xs[3:], axis=1)]
    with torch.no_grad():
        y5 = F_.linear(_linear_inputs(c, xs), c.Ks, weight, bias, act=_ACT[c.act], zero_row0=c.zero_row0)
        y4 = F_.linear(_linear_inputs(c, merged), [m.shape[1] for m in merged], weight, bias, act=_ACT[c.act],
                       zero_row0=c.zero_row0)
    assert rel_err(y5.cpu().numpy(), y4.cpu().numpy()) < C.LINEAR_TOL
