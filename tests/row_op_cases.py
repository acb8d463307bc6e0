"""Case tables and host restatements (numpy) for the CSR builders of csrc/graph.hip and the row movers of csrc/gather.hip
(plus ggpm_sum_slots), run on the GPU by tests/test_row_ops_gpu.py and held to the source by tests/test_row_op_cases_cpu.py.

Everything here is integer work, copies or fp32 sums in a fixed order, so every restatement is exact: the GPU tests compare
bits.  Only the `linear` cases at the end carry a tolerance (the GEMM bar of test_gpu_parity.test_gemm_against_fp64).

No torch and no library import at module level: the tables are plain data that the CPU test can reason about."""
import collections

import numpy as np

# ---------------------------------------------------------------------------------------------- transposes of an index
# csr_from_index(idx, ncols).T: one entry per row.  `lengths`: the number of rows that name each column (the index is those
# ids in shuffled order), None: uniform random ids.  `shuffle`: "all", or "passes": the ids in ascending order shuffled inside
# every run of 1024 rows, the rows the workgroup's 1024 threads handle together in one trip of its loops -- all rows of a
# column then reach its cursor from different waves at the same time, the arrival order that needs the sort most.  `form`: "small" (csr_transpose_small, one workgroup) or "multi" (the six
# launches), chosen by rows / ncols against SMALL_ROWS.  The sort tiers of the small form, by list length n:
#   n <= SORT_SERIAL (24): the thread that owns the column;  n <= SORT_WAVE_CAP (512): one wave through LDS;
#   n <= SORT_PER_THREAD * SCAN_THREADS (16384): the workgroup, in LDS chunks of SORT_BLOCK_CAP (8192): 8193 takes two chunks;
#   more candidates than SORT_LIST (512) of a tier: the surplus is sorted serially (`slot >= SORT_LIST`).
# A second overflow case, more than 512 columns of 513 entries (the workgroup tier's candidate table), cannot be built:
# 513 * 513 rows are far more than the 16 384 the small form takes, so only the wave tier's table can overflow.
IndexCase = collections.namedtuple("IndexCase", "name rows ncols form lengths seed shuffle", defaults=("all",))


def _spread(total, n):
    """`total` rows over `n` columns as evenly as they go"""
    return tuple(total // n + (1 if i < total % n else 0) for i in range(n))


INDEX_SMALL = [
    IndexCase("serial_24_wave_25", 102, 7, "small", (24, 25, 1, 0, 23, 26, 3), 1),
    IndexCase("wave_512_block_513", 1060, 5, "small", (512, 513, 5, 0, 30), 2),
    IndexCase("block_8192_one_chunk", 8192, 1, "small", (8192,), 3),
    IndexCase("block_8193_two_chunks", 8193, 1, "small", (8193,), 4),
    IndexCase("block_16384_full", 16384, 1, "small", (16384,), 5),
    IndexCase("wave_table_overflow", 13000, 520, "small", (25,) * 520, 6, "passes"),
]
# The multi-launch form sorts every list serially (sort_lists): no list here may exceed MULTI_MAX_LIST entries.  The third
# shape is the (rows, 40) case of test_transpose_of_an_index_with_few_ids on this form; there one column holds half the
# rows, which on 20 000 rows would be a 10 000-entry serial sort and seconds of device time, so its long column is held to
# the cap instead (one list of 512 among lists of 499 / 500).
MULTI_MAX_LIST = 512
INDEX_MULTI = [
    IndexCase("multi_rows_16385", 16385, 4097, "multi", None, 7),
    IndexCase("multi_ncols_16385_mostly_empty", 300, 16385, "multi", None, 8),
    IndexCase("multi_20000_one_long_column", 20000, 40, "multi", _spread(19488, 39)[:5] + (512,) + _spread(19488, 39)[5:], 9),
]
assert sum(INDEX_MULTI[2].lengths) == 20000 and len(INDEX_MULTI[2].lengths) == 40


def index_of(c):
    """the int32 index of an IndexCase"""
    rs = np.random.RandomState(c.seed)
    if c.lengths is None:
        return rs.randint(0, c.ncols, size=c.rows).astype(np.int32)
    assert len(c.lengths) == c.ncols and sum(c.lengths) == c.rows, c.name
    idx = np.repeat(np.arange(c.ncols), c.lengths)
    if c.shuffle == "passes":
        for lo in range(0, c.rows, 1024):
            rs.shuffle(idx[lo:lo + 1024])
    else:
        rs.shuffle(idx)
    return idx.astype(np.int32)


def list_lengths(idx, ncols):
    """entries per transposed list; ids outside [0, ncols) are dropped"""
    idx = np.asarray(idx).astype(np.int64)
    return np.bincount(idx[(idx >= 0) & (idx < ncols)], minlength=ncols)


# Dropped ids: the same index with -1 in about a tenth of the rows and some ids at and past ncols, once at the last row count
# of the small form and once, with ONE valid row appended, on the multi-launch form.
DROPPED_NCOLS, DROPPED_ROWS, DROPPED_EXTRA_ID = 300, (16384, 16385), 17


def dropped_index(rows):
    assert rows in DROPPED_ROWS
    rs = np.random.RandomState(10)
    n = DROPPED_ROWS[0]
    idx = rs.randint(0, DROPPED_NCOLS, size=n).astype(np.int64)
    idx[rs.rand(n) < 0.10] = -1
    bad = rs.choice(n, size=200, replace=False)
    idx[bad] = np.resize([DROPPED_NCOLS, DROPPED_NCOLS + 5, -7, 2 ** 31 - 1, -2 ** 31], 200)
    idx[0], idx[n - 1] = -1, DROPPED_NCOLS          # a dropped entry in the first and in the last shared row
    if rows > n:
        idx = np.concatenate([idx, [DROPPED_EXTRA_ID]])
    return idx.astype(np.int32)


def transpose_ref(rowptr, col, rows, ncols):
    """-> (rowptrT [ncols + 1], colT [number of in-range entries]): per column id the ascending list of the rows that name
    it, a row as often as it names it.  Entries outside [0, ncols) are dropped."""
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)[: int(rowptr[-1])]
    row_of = np.repeat(np.arange(rows), np.diff(rowptr))
    ok = (col >= 0) & (col < ncols)
    order = np.argsort(col[ok], kind="stable")          # stable: rows stay ascending inside a column
    rowptrT = np.concatenate([[0], np.cumsum(np.bincount(col[ok], minlength=ncols))])
    return rowptrT.astype(np.int32), row_of[ok][order].astype(np.int32)


def index_transpose_ref(idx, ncols):
    idx = np.asarray(idx)
    return transpose_ref(np.arange(idx.size + 1), idx, idx.size, ncols)


# ---------------------------------------------------------------------------------------------- padded tables
# csr_from_padded: int64 [rows, width], 0 = no entry.  Rows at, one past and well past SMALL_ROWS; ncols small enough that the
# transpose of the 16 384-row tables stays on the small form while the others take the multi-launch one (through rows).
# Values stay below 2^31: include/ggpm_hip.h promises nothing about wider ones.
PaddedCase = collections.namedtuple("PaddedCase", "rows width ncols seed")
PADDED = [PaddedCase(rows, width, 4096, rows + width) for rows in (16384, 16385, 20000) for width in (1, 5)]
PADDED_PAIR = [(PaddedCase(16385, 3, 4096, 21), PaddedCase(7, 2, 50, 22)), (PaddedCase(9, 4, 50, 23), PaddedCase(16385, 1, 4096, 24))]


def padded_of(c):
    """random ids in [1, ncols) with about half the slots empty (zeros anywhere in a row, not only at its end); at both ends
    of the table a row of zeros, a full row and, where the width allows, a zero between two entries"""
    rs = np.random.RandomState(c.seed)
    p = rs.randint(1, c.ncols, size=(c.rows, c.width)).astype(np.int64)
    p[rs.rand(c.rows, c.width) < 0.5] = 0
    full = np.arange(1, c.width + 1, dtype=np.int64) * 7 % (c.ncols - 1) + 1
    holed = full.copy()
    holed[1::2] = 0                                      # [8, 0, 22, 0, 36]: width 1 has no middle
    if c.rows >= 6:
        p[0], p[1], p[2] = 0, full, holed
        p[-1], p[-2], p[-3] = full, 0, holed
    return p


def padded_csr_ref(padded):
    """-> (rowptr [rows + 1], col [number of non-zero entries]), entries in their in-row order"""
    mask = padded != 0
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))])
    return rowptr.astype(np.int32), padded[mask].astype(np.int32)


# ---------------------------------------------------------------------------------------------- ggpm_segment_sum
# out[r, :width] = (accumulate ? out[r, :width] : 0) + src[col[j], :width] for j = rowptr[r] .. rowptr[r + 1] - 1, one fp32
# addition after the other in list order; columns [width, zero_to) of every row are set to 0.  One wave per row, four rows per
# workgroup; 16-byte accesses over 256 columns per trip when all five SEG_CONDITIONS hold, 64 scalar columns per trip otherwise.
# src_off / out_off: floats between the (16-byte aligned) allocation and the first element: 1 misaligns the base by 4 bytes.
# lists: "mixed" (0, 1, 2 equal, 5 with a repeat, 3, ... entries), "long" (the last row lists 9 000 entries), "shared" (mixed,
# and the lists of three and four entries begin with the source row that the first list names).
# twin: the aligned case with the same values and lists whose columns the scalar result must repeat bit for bit.
SegCase = collections.namedtuple("SegCase", "name rows width nsrc ld_src ld_out src_off out_off accumulate zero_to lists seed twin")
SEG_CONDITIONS = ("width", "ld_src", "ld_out", "src", "out")
SEG_VALUE_COLUMNS = 304          # every case draws [*, 304] values and uses the first `width` columns: twins share values
LONG_LIST = 9000


def seg_broken(c):
    """the alignment conditions of ggpm_segment_sum's `vec` that the case fails (none: the 16-byte kernel runs)"""
    fails = (c.width % 4, c.ld_src % 4, c.ld_out % 4, c.src_off % 4, c.out_off % 4)
    return tuple(n for n, f in zip(SEG_CONDITIONS, fails) if f)


def _seg(name, rows, width, accumulate, zero_to, lists="mixed", seed=None, nsrc=37, ld_src=None, ld_out=None, src_off=0,
         out_off=0, twin=None):
    ld = (width + 3) // 4 * 4 + 8
    ld_src, ld_out = ld_src or ld, ld_out or ld
    zt = {"width": width, "width+1": width + 1, "ld": ld_out, "none": 0}[zero_to]
    return SegCase(name, rows, width, nsrc, ld_src, ld_out, src_off, out_off, accumulate, zt, lists,
                   seed if seed is not None else rows * 1000 + width, twin)


SEGMENT_SUM = [
    _seg("r1_w1", 1, 1, 0, "width"),
    _seg("r3_w3_acc", 3, 3, 1, "width+1"),
    _seg("r4_w4", 4, 4, 0, "ld"),
    _seg("r5_w64_acc", 5, 64, 1, "none"),
    _seg("r201_w252", 201, 252, 0, "width+1"),
    _seg("r5_w256_acc", 5, 256, 1, "ld"),
    _seg("r201_w260", 201, 260, 0, "none"),
    _seg("r201_w300_acc", 201, 300, 1, "width"),
    _seg("r4_w1_acc", 4, 1, 1, "ld"),
    _seg("r5_w3", 5, 3, 0, "none"),
    _seg("r3_w300", 3, 300, 0, "ld"),
    _seg("long_w64_acc", 5, 64, 1, "ld", lists="long"),
    _seg("long_w3", 3, 3, 0, "width+1", lists="long"),
    # the aligned twin and the five cases that each fail ONE condition of `vec` on the same values and lists
    _seg("twin_w260", 5, 260, 1, "ld", seed=77, ld_src=272, ld_out=268),
    _seg("break_width", 5, 259, 1, "ld", seed=77, ld_src=272, ld_out=268, twin="twin_w260"),
    _seg("break_ld_src", 5, 260, 1, "ld", seed=77, ld_src=273, ld_out=268, twin="twin_w260"),
    _seg("break_ld_out", 5, 260, 1, "ld", seed=77, ld_src=272, ld_out=269, twin="twin_w260"),
    _seg("break_src", 5, 260, 1, "ld", seed=77, ld_src=272, ld_out=268, src_off=1, twin="twin_w260"),
    _seg("break_out", 5, 260, 1, "ld", seed=77, ld_src=272, ld_out=268, out_off=1, twin="twin_w260"),
]
# a NaN and an Inf in ONE source row (SEG_SPECIAL_COLUMNS of the row that the first list names first), 16-byte and scalar form
SEGMENT_SUM_SPECIAL = [_seg("special_w64", 9, 64, 0, "ld", lists="shared"), _seg("special_w63_acc", 9, 63, 1, "ld", lists="shared")]
SEG_SPECIAL_COLUMNS = (2, 5)     # NaN, +Inf


def seg_case(name):
    return next(c for c in SEGMENT_SUM if c.name == name)


def seg_lists(c):
    """-> (rowptr, col) int32 of the case's lists; rows r % 8 == 2 name one source row twice, lists of five repeat an entry"""
    rs = np.random.RandomState(c.seed % 1000 + 5)
    lens = [(1, 0, 2, 5, 3, 1, 0, 4)[r % 8] for r in range(c.rows)]
    if c.lists == "long":
        lens[-1] = LONG_LIST
    col = []
    for n in lens:
        ids = rs.randint(0, c.nsrc, size=n)
        if c.lists == "shared" and n in (3, 4):
            ids[0] = col[0][0]
        if n == 2:
            ids[1] = ids[0]
        if n == 5:
            ids[3] = ids[1]
        col.append(ids)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    return rowptr.astype(np.int32), (np.concatenate(col) if col else np.zeros(0)).astype(np.int32)


def seg_values(c):
    """-> (src [nsrc, width], the values `out` holds before an accumulating call [rows, width]) float32"""
    rs = np.random.RandomState(c.seed)
    src = rs.standard_normal((c.nsrc, SEG_VALUE_COLUMNS)).astype(np.float32)
    old = rs.standard_normal((c.rows, SEG_VALUE_COLUMNS)).astype(np.float32)
    return src[:, :c.width].copy(), old[:, :c.width].copy()


def segment_sum_ref(src, rowptr, col, width, out, accumulate, zero_to):
    """ggpm_segment_sum on host arrays: `out` [rows, ld_out] is updated in place (float32, one addition per entry, in list
    order, every column for itself) and returned"""
    assert src.dtype == np.float32 and out.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(rowptr) - 1):
            acc = out[r, :width].copy() if accumulate else np.zeros(width, dtype=np.float32)
            for j in range(int(rowptr[r]), int(rowptr[r + 1])):
                acc = acc + src[col[j], :width]            # float32 + float32: rounded once, as the kernel's v_add_f32
            out[r, :width] = acc
            if zero_to > width:
                out[r, width:zero_to] = 0.0
    return out


# ---------------------------------------------------------------------------------------------- ggpm_gather_rows
# out[r, col_off : col_off + width] = table[idx[r], :width] (idx < 0: zeros); columns [col_off + width, zero_to) zeroed
GatherCase = collections.namedtuple("GatherCase", "rows width col_off zero_to first_negative")
GATHER_NTAB = 11


def gather_geometry(c):
    """-> (ld_table > width, ld_out, zero_to as a column)"""
    ld_out = c.col_off + c.width + 7
    return c.width + 3, ld_out, {"none": 0, "end": c.col_off + c.width, "ld": ld_out}[c.zero_to]


GATHER = [
    GatherCase(1, 1, 0, "none", False), GatherCase(1, 63, 5, "ld", True), GatherCase(1, 300, 0, "ld", False),
    GatherCase(5, 64, 0, "end", False), GatherCase(5, 65, 5, "none", False), GatherCase(5, 1, 5, "ld", False),
    GatherCase(401, 300, 5, "ld", False), GatherCase(401, 63, 0, "ld", False), GatherCase(401, 64, 5, "end", False),
    GatherCase(401, 65, 0, "none", False),
]


def gather_index(c):
    """ids into a table of GATHER_NTAB rows: repeats everywhere, -1 in every fourth row"""
    rs = np.random.RandomState(c.rows + c.width)
    idx = rs.randint(0, GATHER_NTAB, size=c.rows)
    if c.rows >= 3:
        idx[2] = idx[1]
        idx[::4] = -1
    elif c.first_negative:
        idx[0] = -1
    return idx.astype(np.int32)


def gather_rows_ref(table, idx, width, out, col_off, zero_to):
    """ggpm_gather_rows on host arrays: `out` is updated in place and returned"""
    for r, i in enumerate(idx):
        out[r, col_off:col_off + width] = table[i, :width] if i >= 0 else 0.0
        if zero_to > col_off + width:
            out[r, col_off + width:zero_to] = 0.0
    return out


# ---------------------------------------------------------------------------------------------- ggpm_onehot
# out[r, col_off + c] = (idx[r] == c) for c < classes; columns [col_off + classes, zero_to) zeroed; 64 columns per workgroup
OnehotCase = collections.namedtuple("OnehotCase", "classes col_off zero_to")      # zero_to relative to col_off + classes
ONEHOT = [
    OnehotCase(1, 0, None), OnehotCase(1, 300, 64), OnehotCase(20, 0, -15), OnehotCase(20, 300, 4), OnehotCase(64, 0, 0),
    OnehotCase(64, 300, 70), OnehotCase(65, 0, 3), OnehotCase(65, 300, -55), OnehotCase(130, 0, 0), OnehotCase(130, 300, 1),
]
ONEHOT_ROWS = 9


def onehot_geometry(c):
    """-> (ld_out, zero_to as a column; None in the table: 0, "leave the pad alone")"""
    end = c.col_off + c.classes
    zero_to = 0 if c.zero_to is None else end + c.zero_to
    return max(end, zero_to) + 5, zero_to


def onehot_index(c):
    """ONEHOT_ROWS ids: below 0, first, last, `classes` itself (one past), far past, and ids in between"""
    k = c.classes
    return np.array([-1, 0, k - 1, k, k // 2, k + 64, -k, k // 3, 2 ** 31 - 1], dtype=np.int32)


def onehot_ref(idx, classes, out, col_off, zero_to):
    for r, i in enumerate(idx):
        out[r, col_off:col_off + classes] = 0.0
        if 0 <= i < classes:
            out[r, col_off + i] = 1.0
        if zero_to > col_off + classes:
            out[r, col_off + classes:zero_to] = 0.0
    return out


# ---------------------------------------------------------------------------------------------- ggpm_embed_graph
# hnode[N1, ld_n] = onehot(fnode); hmess[E1, ld_m] = [onehot(fnode[fmess[:, 0]]) | onehot(fmess[:, 2]) | onehot(fmess[:, 3])],
# every column up to the leading dimension written (pad columns zero); one 256-thread workgroup per row: ld <= 256.
# rc: 0 GGPM_OK, 3 GGPM_ERR_UNSUPPORTED (nothing written).
EmbedCase = collections.namedtuple("EmbedCase", "name N1 E1 atom bond pos ld_n ld_m rc")


def _ceil4(n):
    return (n + 3) // 4 * 4


EMBED = [
    EmbedCase("one_row_each", 1, 1, 37, 4, 20, 40, 64, 0),
    EmbedCase("product_ld", 23, 50, 37, 4, 20, _ceil4(37), _ceil4(61), 0),
    EmbedCase("wide_ld", 23, 50, 37, 4, 20, 48, 72, 0),
    EmbedCase("message_width_256", 9, 14, 232, 4, 20, 232, 256, 0),
    EmbedCase("node_width_256", 9, 14, 256, 0, 0, 256, 256, 0),
    EmbedCase("message_width_257", 9, 14, 233, 4, 20, 236, 260, 3),
    EmbedCase("message_width_257_ld_256", 9, 14, 233, 4, 20, 236, 256, 3),
    EmbedCase("node_width_257", 9, 14, 257, 0, 0, 260, 260, 3),
    EmbedCase("ld_n_below_width", 9, 14, 37, 4, 20, 36, 64, 3),
    EmbedCase("ld_m_below_width", 9, 14, 37, 4, 20, 40, 60, 3),
]


def embed_inputs(c):
    """-> (fnode int64 [N1], fmess int64 [E1, 4]); atom types, bond types and positions in range except for the marked rows:
    an atom type of -1 and of `atom`, a bond type of -1 and of `bond`, a position of -1 and of `pos`"""
    rs = np.random.RandomState(c.N1 * 100 + c.E1)
    fnode = rs.randint(0, c.atom, size=c.N1).astype(np.int64)
    fmess = np.zeros((c.E1, 4), dtype=np.int64)
    fmess[:, 0] = rs.randint(0, c.N1, size=c.E1)
    fmess[:, 1] = rs.randint(0, c.N1, size=c.E1)
    fmess[:, 2] = rs.randint(0, max(c.bond, 1), size=c.E1)
    fmess[:, 3] = rs.randint(0, max(c.pos, 1), size=c.E1)
    if c.N1 > 4:
        fnode[1], fnode[2], fnode[3] = -1, c.atom, c.atom - 1
        fmess[0, 0], fmess[1, 0], fmess[2, 0] = 1, 2, 3          # messages whose source atom has no / the last type
    if c.E1 > 8:
        fmess[3, 2], fmess[4, 2], fmess[5, 2] = -1, c.bond, max(c.bond - 1, 0)
        fmess[6, 3], fmess[7, 3], fmess[8, 3] = -1, c.pos, max(c.pos - 1, 0)
    return fnode, fmess


def embed_graph_ref(fnode, fmess, atom, bond, pos, ld_n, ld_m):
    hnode = np.zeros((len(fnode), ld_n), dtype=np.float32)
    hmess = np.zeros((len(fmess), ld_m), dtype=np.float32)
    for r, a in enumerate(fnode):
        if 0 <= a < atom:
            hnode[r, a] = 1.0
    for e, f in enumerate(fmess):
        a = fnode[f[0]]
        if 0 <= a < atom:
            hmess[e, a] = 1.0
        if 0 <= f[2] < bond:
            hmess[e, atom + f[2]] = 1.0
        if 0 <= f[3] < pos:
            hmess[e, atom + bond + f[3]] = 1.0
    return hnode, hmess


# ---------------------------------------------------------------------------------------------- ggpm_sum_slots
# out[i] = src[0][i] + src[1][i] + ... + src[slots - 1][i]: sum_slots_k (csrc/mpn_gru.hip) starts from slot 0 and adds the
# slots upwards, one fp32 addition each; 16 bytes per thread, 256 threads per workgroup (1028 floats: a second workgroup).
SUM_SLOTS = [(slots, n) for slots in (1, 2, 7) for n in (4, 1024, 1028)]
SUM_SLOTS_REFUSED = (6, 1023, 0)          # slot_floats that are no positive multiple of 4


def sum_slots_ref(src):
    """src [slots, slot_floats] float32 -> the sum over slots in index order"""
    acc = src[0].copy()
    for t in range(1, src.shape[0]):
        acc = acc + src[t]
    return acc


# ---------------------------------------------------------------------------------------------- functional.linear
# y[:, :N] = act(sum_i x_i[:, :K_i] W[:, off_i : off_i + K_i]^T + b): one GEMM for one input, gemm_ksegments for 2-4, an
# accumulate chain of GEMMs for more (`route`).  Segment widths from {24, 38, 62, 300}: 24 and 300 keep the next weight slice
# 16-byte aligned, 38 and 62 do not.  ld_out_extra: columns beyond padded_hidden(N); ld_x_extra: columns of every input beyond
# its K (they hold NaN).  Bar: LINEAR_TOL on max|got - ref| / max|ref| against fp64, the bar of test_gemm_against_fp64 for
# K <= 5000 (every K here is below 500).
LinearCase = collections.namedtuple("LinearCase", "name M N Ks act zero_row0 bias ld_out_extra ld_x_extra")
LINEAR_TOL = 2e-6
LINEAR_WIDTHS = (24, 38, 62, 300)
LINEAR = [
    LinearCase("one_segment", 17, 33, (62,), "none", False, True, 0, 4),
    LinearCase("one_segment_tanh_row0", 130, 20, (300,), "tanh", True, True, 16, 0),
    LinearCase("two_segments_relu", 17, 300, (24, 38), "relu", False, True, 0, 3),
    LinearCase("two_segments_no_bias", 1, 33, (62, 300), "none", False, False, 16, 4),
    LinearCase("four_segments_relu_row0", 130, 33, (24, 38, 62, 300), "relu", True, True, 0, 4),
    LinearCase("four_segments_tanh_no_bias", 17, 8, (38, 38, 24, 62), "tanh", False, False, 16, 0),
    LinearCase("five_segments_relu_row0", 130, 33, (24, 38, 62, 300, 24), "relu", True, True, 0, 4),
    LinearCase("five_segments_plain_no_bias", 17, 300, (38, 24, 62, 24, 38), "none", False, False, 16, 4),
    LinearCase("five_segments_tanh_one_row", 1, 20, (24, 38, 62, 300, 38), "tanh", False, True, 0, 3),
]
GRADIENT_ROUTES = [("1", "1"), ("0", "1"), ("0", "0")]       # GGPM_DEFER_WGRADS, GGPM_SIDE_STREAM
GRADIENT_ROUTE_IDS = ["deferred", "second_stream", "main_stream"]


def linear_route(c):
    n = len(c.Ks)
    return "gemm" if n == 1 else "ksegments" if n <= 4 else "chain"


def linear_values(c):
    """-> (xs [M, K_i] each, W [N, sum K], b [N], upstream gradient [M, N]) float32"""
    rs = np.random.RandomState(c.M * 31 + c.N * 7 + len(c.Ks))
    xs = [rs.standard_normal((c.M, K)).astype(np.float32) for K in c.Ks]
    W = (rs.standard_normal((c.N, sum(c.Ks))) / np.sqrt(sum(c.Ks))).astype(np.float32)
    b = rs.standard_normal(c.N).astype(np.float32)
    g = rs.standard_normal((c.M, c.N)).astype(np.float32)
    return xs, W, b, g


# ---------------------------------------------------------------------------------------------- the index wrappers
# functional.segment_sum / gather_rows / tree_message_input: `H` columns of a table inside a wider buffer, `width` < H of them
# moved; ids that no row names.  Their backward walks the transposed lists in ascending row order: segment_sum_ref on
# transpose_ref's lists restates it exactly.
WrapperCase = collections.namedtuple("WrapperCase", "rows nsrc H width ld seed")
WRAPPERS = [WrapperCase(5, 9, 12, 8, 16, 31), WrapperCase(203, 50, 70, 65, 80, 32), WrapperCase(130, 400, 300, 260, 304, 33)]
TREE_POSITIONS = 20


def wrapper_index(c):
    """ids in [0, nsrc) that leave the ids 3 and nsrc - 1 (and, with more ids than rows, many others) unused"""
    rs = np.random.RandomState(c.seed)
    idx = rs.randint(0, c.nsrc - 1, size=c.rows)
    idx[idx == 3] = 4
    return idx.astype(np.int32)


def wrapper_lists(c):
    """-> (rowptr, col) of a segment_sum over `nsrc` source rows: 0 .. 4 entries per row, repeats allowed, ids 3 and
    nsrc - 1 unused"""
    rs = np.random.RandomState(c.seed + 100)
    lens = rs.randint(0, 5, size=c.rows)
    lens[1] = 0
    col = rs.randint(0, c.nsrc - 1, size=int(lens.sum()))
    col[col == 3] = 4
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), col.astype(np.int32)
