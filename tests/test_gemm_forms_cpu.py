"""CPU: ggpm_gemm_form_query (host only) against the case table of tests/gemm_form_cases.py -- every case takes the form
the table states, every form a lattice of shapes, transposes, alignments, workspaces and group sizes reaches has a case
that tests/test_gpu_gemm_forms.py runs against fp64, no form exceeds the LDS of a workgroup or HIP's grid limits, and the
workspace queries cover what the chosen form writes."""
import ctypes
import itertools

import gemm_form_cases as C
from ggpm_amd import _lib
from ggpm_amd import functional as F_

LDS_BYTES = 160 * 1024
GRID_MAX = (2 ** 31 - 1, 65535, 65535)

LAT_M = (1, 33, 64, 65, 160, 161, 250, 300, 573, 600, 2751, 2843)
LAT_N = (1, 16, 62, 64, 65, 250, 300, 340, 600, 912)
LAT_K = (1, 31, 32, 62, 64, 65, 300, 2047, 2048, 2848, 6143, 6144, 9001, 20000, 57011)
ALIGN = (("v", "v"), ("v", "l"), ("l", "v"), ("l", "l"))
WS = ("none", "exact", "slab", "short")


def _table():
    return {C.form_key(c.entry, C.expected(c)) for c in C.CASES + C.REFUSALS}


def test_every_case_takes_the_form_the_table_states():
    bad = [(c.name, C.reduced(c), C.expected(c)) for c in C.CASES + C.REFUSALS if C.reduced(c) != C.expected(c)]
    assert not bad, "%d cases, first: %r" % (len(bad), bad[:5])


def test_case_names_are_unique_and_the_named_cases_stay():
    names = [c.name for c in C.CASES + C.REFUSALS]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    for prefix in C.NAMED:
        assert any(n.startswith(prefix + "-") for n in names), "the named case %r left the table" % prefix
    by = {}
    for c in C.CASES:
        by.setdefault(c.name.split("-" + c.entry + "-")[0], []).append(c)
    # what the named cases are there for
    assert {(c.ta, c.tb, c.va, c.vb) for c in by["scalar"]} == {t + v for t in C.TRANS for v in (("l", "l"), ("v", "l"), ("l", "v"))}
    assert {c.va + c.vb for c in by["scalar-base"]} == {"1v", "2v", "3v", "v1", "v2", "v3"}
    assert {c.K for c in by["v2-steps"]} == {63, 127, 128, 129} and {c.K for c in by["v2"]} == {64, 65}
    assert C.cdiv(by["v3-300-tiles"][0].M, 64) * C.cdiv(by["v3-300-tiles"][0].N, 64) == C.SMALL_TILES
    assert C.cdiv(by["v3-301-tiles"][0].M, 64) * C.cdiv(by["v3-301-tiles"][0].N, 64) == C.SMALL_TILES + 1
    assert C.cdiv(by["resident-512"][0].M, 64) * C.cdiv(by["resident-512"][0].N, 64) == C.RESIDENT_WGS
    assert by["splitk-2047"][0].K == C.SPLITK_K - 1 and by["splitk-2048"][0].K == C.SPLITK_K
    assert C.ws_bytes(by["splitk-short-ws"][0]) == C.choose_splits(65, 65, 2048) * 65 * 65 * 4 - 1
    assert by["tall-K-6143"][0].K == C.TALL_K - 1 and (by["tall-cover-0.8"][0].M, by["tall-cover-0.8"][0].N) == (160, 128)
    assert {(c.count, c.mode) for c in by["tall-group"]} == {(n, m) for n in (1, 2, 3, 4) for m in (0, 1, 2)} - {(1, 0)}
    for c in by["tall-group"]:           # a member with fewer K chunks than the group: its last slabs are written as zeros
        f = C.query(c)
        assert c.count == 1 or any(C.cdiv(k, f.k_chunk[i]) < f.splits for i, k in enumerate(C.ks(c))), (c.name, f.splits)
    for c in by["group-splitk-last-chunk-of-one"]:
        f = C.query(c)
        assert c.K - (f.splits - 1) * f.k_chunk[0] == 1, (c.name, f.splits, f.k_chunk[0])
    assert {c.count for c in by["pairs"]} == {1, 2, 3, 4} and {c.count for c in by["segs-scalar"]} == {2, 3, 4}
    assert sorted({k for c in by["segs-scalar"] for k in c.K}) == [1, 32, 63, 65]


def _lattice_calls():
    """(entry, ta, tb, M, N, Ks, count, va, vb, ws, mode) over the lattice of the issue"""
    shapes = list(itertools.product(LAT_M, LAT_N, LAT_K))
    for (M, N, K), (ta, tb), (va, vb), ws in itertools.product(shapes, C.TRANS, ALIGN, WS):
        yield ("gemm", ta, tb, M, N, K, 1, va, vb, ws, 0)
    for (M, N, K), count, (va, vb) in itertools.product(shapes, (1, 2, 3, 4), ALIGN + (("vl", "v"),)):
        for ta, tb in C.TRANS:
            yield ("grouped", ta, tb, M, N, K, count, va, vb, "none", 0)
            for ws in ("exact", 1024):
                yield ("grouped_splitk", ta, tb, M, N, K, count, va, vb, ws, 0)
        for tb in (0, 1):
            yield ("ksegments", 0, tb, M, N, (K, 64, 63, 1)[:count], count, va, vb, "none", 0)
        for ws, mode in itertools.product(("none", "slab", "full"), (0, 1, 2)):
            yield ("tall_grouped", 1, 0, M, N, (K, K + 31, K + 1, K + 32)[:count], count, va, vb, ws, mode)


def _lattice_forms():
    """-> {(entry, reduced form): first call that took it}, with every form checked for its limits on the way"""
    seen = {}
    lib, out = _lib.load(), F_.GemmForm()
    for entry, ta, tb, M, N, K, count, va, vb, ws, mode in _lattice_calls():
        c = C.Case("lattice", entry, ta, tb, M, N, K, count, va, vb, None, 3, ws, mode, None, None, None, None)
        if ws == "short" and C.choose_splits(M, N, K) == 1:
            continue                                   # nothing to be one byte short of
        f = C.query(c, out)
        Ks = C.ks(c) if entry in ("ksegments", "tall_grouped") else C.ks(c)[:1]
        key = C.form_key(entry, C.reduce_form(entry, ta, tb, M, N, Ks, count, f))
        seen.setdefault(key, (entry, ta, tb, M, N, K, count, va, vb, ws, mode))
        what = (entry, ta, tb, M, N, K, count, va, vb, ws, mode)
        assert f.lds_bytes <= LDS_BYTES, what
        assert all(0 <= f.grid[i] <= GRID_MAX[i] for i in range(3)), (what, list(f.grid))
        passed = C.ws_bytes(c)
        assert f.ws_used <= (passed or 0), (what, f.ws_used, passed)
        if entry == "gemm":
            assert f.ws_used <= lib.ggpm_gemm_workspace_bytes(M, N, K) or ws in ("slab",), (what, f.ws_used)
        if entry == "grouped_splitk":
            assert f.ws_used <= lib.ggpm_gemm_grouped_splitk_workspace_bytes(M, N, K, count), (what, f.ws_used)
    return seen


def test_every_form_the_lattice_reaches_has_a_case():
    table = _table()
    missing = sorted((k, v) for k, v in _lattice_forms().items() if k not in table and k[1] != "refused")
    assert not missing, "%d forms without a case; first (entry + form, a call that takes it): %r" % (len(missing), missing[:3])


def test_the_workspace_queries_cover_the_full_workspace_forms():
    """ggpm_gemm with exactly ggpm_gemm_workspace_bytes(M, N, K): whichever kernel, the slabs it writes fit -- and a tall
    shape given that much does split (the query leaves room for either tall kernel)"""
    lib = _lib.load()
    for M, N, K in itertools.product(LAT_M, LAT_N, LAT_K):
        need = int(lib.ggpm_gemm_workspace_bytes(M, N, K))
        for (ta, tb), (va, vb) in itertools.product(C.TRANS, ALIGN):
            c = C.Case("ws", "gemm", ta, tb, M, N, K, 1, va, vb, None, 3, need or "none", 0, None, None, None, None)
            f = C.query(c)
            assert f.rc == C.OK and f.ws_used <= need, (M, N, K, ta, tb, va, vb, f.ws_used, need)


def test_the_query_refuses_what_it_cannot_describe():
    lib = _lib.load()
    call, out = F_.GemmCall(), F_.GemmForm()
    assert lib.ggpm_gemm_form_query(None, ctypes.byref(out)) == C.ERR_ARG
    assert lib.ggpm_gemm_form_query(ctypes.byref(call), None) == C.ERR_ARG
    call.entry = len(F_.GEMM_ENTRIES)
    assert lib.ggpm_gemm_form_query(ctypes.byref(call), ctypes.byref(out)) == C.ERR_ARG


def test_tall_operands_leave_room_for_the_k_overshoot_below_4_gib():
    """The tall kernels' 32-bit buffer offsets run up to three 32-row steps past K: an operand whose K rows end within that
    of 4 GiB must not take them (the offsets of the K tail would wrap into the operand's start)."""
    ld = 174760                                   # 6144 rows of ld floats: 0xffff0000 bytes, under the 0xffffff00 limit
    assert 6144 * ld * 4 < 0xffffff00 < (6144 + 96) * ld * 4
    tall = {"gemm_tn_tall", "gemm_tn_tall_split", "gemm_tn_tall_bf16<false>", "gemm_tn_tall_bf16<true>"}
    for lda, ldb in ((ld, 164), (164, ld)):
        f = F_.gemm_form("gemm", 1, 0, 160, 160, 6144, lda, ldb, 163, 160, ws_bytes=1 << 30)
        assert f.rc == C.OK and F_.GEMM_KERNELS[f.kernel] not in tall, F_.GEMM_KERNELS[f.kernel]
        f = F_.gemm_form("tall_grouped", 1, 0, 160, 160, [6144] * 4, lda, ldb, 163, 160, count=2, ws_bytes=1 << 30, mode=1)
        assert F_.GEMM_KERNELS[f.kernel] == "sequence"
    f = F_.gemm_form("gemm", 1, 0, 160, 160, 6144, ld - 2800, 164, 163, 160, ws_bytes=1 << 30)
    assert F_.GEMM_KERNELS[f.kernel] == "gemm_tn_tall_split"
