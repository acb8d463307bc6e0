"""The case table of the GEMM family (csrc/gemm.hip): one case per form a call can take.

A case names an entry point, its arguments and the kernel / split / reduce it must run on; tests/test_gemm_forms_cpu.py
holds the table against ggpm_gemm_form_query (host only) and against a lattice of shapes, tests/test_gpu_gemm_forms.py
runs every case against fp64 with poisoned padding.  Shapes are the smallest that reach the form, not the workload's.

Operand layout of a case.  A'(m, k) is read from a [rows_a x lda] matrix (rows_a = K if ta else M, logical width M if ta
else K), B'(k, n) likewise.  `va` / `vb` say whether 16-byte loads are legal and, if not, why:
    "v"  legal: ld % 4 == 0, base 16-byte aligned          "l"  illegal by leading dimension: ld % 4 == 1
    "1", "2", "3"  illegal by base: ld % 4 == 0, the base offset by that many floats
per member ("vl": member 0 legal, member 1 not).  `ws`: "none" (no pointer), "exact" (what the *_workspace_bytes query
says), "short" (one byte under the plain split-K need), "underslab" / "slab" (one byte under / exactly count tall slabs),
"full" (count x ggpm_gemm_workspace_bytes of the longest member) or a number of bytes.
"""
import collections
import ctypes
import functools

from ggpm_amd import _lib
from ggpm_amd import functional as F_

Case = collections.namedtuple("Case", "name entry ta tb M N K count va vb n_pad ldc_extra ws mode kernel split reduce rc")

# tile (rows, columns) and k-step of each kernel: what "ragged" is measured against (csrc/gemm.hip: BM/BN/BK, BK2, SM/SN/SK,
# TM/TN/TK, BTK)
TILES = {"gemm_kernel": (64, 64, 32), "gemm_kernel_segs": (64, 64, 32), "gemm_kernel_group": (64, 64, 32),
         "gemm_kernel_v2": (64, 64, 64), "gemm_group_v2": (64, 64, 64), "gemm_small_v3": (32, 32, 64),
         "gemm_tn_tall": (160, 160, 16), "gemm_tn_tall_bf16<false>": (160, 160, 32), "gemm_tn_tall_bf16<true>": (160, 160, 32),
         "gemm_tn_tall_split": (160, 160, 32)}
SMALL_TILES, RESIDENT_WGS = 300, 512            # small_launch; the resident limit of gemm_kernel_v2
TALL_K, TALL_COVER = 6144, 0.8                  # tall_shape
SPLITK_K, SPLITK_TILES = 2048, 512              # choose_splits
OK, ERR_ARG, ERR_UNSUPPORTED = _lib.GGPM_OK, _lib.GGPM_ERR_ARG, _lib.GGPM_ERR_UNSUPPORTED


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def ks(c):
    """K per member / segment"""
    return tuple(c.K) if isinstance(c.K, tuple) else (c.K,) * max(c.count, 1)


def members(c, s):
    return (s * c.count)[:c.count] if len(s) < c.count else s


def ld_of(width, v):
    """leading dimension of an operand of logical width `width` under legality code v: always wider than the matrix"""
    return rup(width, 4) + (5 if v == "l" else 4)


def off_of(v):
    return int(v) if v in "123" else 0


def geometry(c):
    """-> per member lists lda, ldb, ldc, n_pad, base_a, base_b (low four address bits) of the call the case makes"""
    K = ks(c)
    es = 2 if c.mode == 2 else 4
    lda, ldb, ldc, n_pad, ba, bb = [], [], [], [], [], []
    for i in range(min(c.count, 4)):
        va, vb = members(c, c.va)[i], members(c, c.vb)[i]
        if c.entry == "pair_grouped":
            wa = wb = max(c.M, c.N)
        elif c.entry == "ksegments":
            wa, wb = K[i], (K[i] if c.tb else c.N)
        else:
            k = K[i] if c.entry in ("tall_grouped",) else K[0]
            wa, wb = (c.M if c.ta else k), (k if c.tb else c.N)
        lda.append(ld_of(wa, va)); ldb.append(ld_of(wb, vb))
        ba.append(off_of(va) * es % 16); bb.append(off_of(vb) * es % 16)
        npd = c.n_pad[i] if isinstance(c.n_pad, tuple) else c.n_pad
        npd = c.N if npd is None else npd
        n_pad.append(npd)
        ldc.append(max(npd, c.N) + c.ldc_extra)
    return lda, ldb, ldc, n_pad, ba, bb


def choose_splits(M, N, K):
    """plain split-K of ggpm_gemm (csrc/gemm.hip: choose_splits), for the "short" workspace"""
    tiles = cdiv(M, 64) * cdiv(N, 64)
    if K < SPLITK_K or tiles >= SPLITK_TILES:
        return 1
    return max(1, min(cdiv(1024, tiles), K // 256))


def slab_bytes(M, N):
    return cdiv(M, 160) * cdiv(N, 160) * 4 * 25 * 64 * 16


_LIB = functools.lru_cache(None)(_lib.load)


def ws_bytes(c):
    """-> None (no workspace pointer) or the bytes passed"""
    if c.ws == "none":
        return None
    if isinstance(c.ws, int):
        return c.ws
    lib, K = _LIB(), ks(c)
    if c.ws == "exact":
        if c.entry == "grouped_splitk":
            b = int(lib.ggpm_gemm_grouped_splitk_workspace_bytes(c.M, c.N, K[0], c.count))
        else:
            b = int(lib.ggpm_gemm_workspace_bytes(c.M, c.N, max(K)))
        return b or None
    if c.ws == "short":
        return choose_splits(c.M, c.N, K[0]) * c.M * c.N * 4 - 1
    if c.ws == "slab":
        return c.count * slab_bytes(c.M, c.N)
    if c.ws == "underslab":
        return c.count * slab_bytes(c.M, c.N) - 1
    assert c.ws == "full", c.ws
    return c.count * max(int(lib.ggpm_gemm_workspace_bytes(c.M, c.N, max(K))), slab_bytes(c.M, c.N))


_CALL = F_.GemmCall()
_ENTRY = {e: i for i, e in enumerate(F_.GEMM_ENTRIES)}


def query(c, out=None):
    """ggpm_gemm_form_query of the call the case makes (out: a GemmForm to reuse)"""
    lda, ldb, ldc, n_pad, ba, bb = geometry(c)
    call, K, wsb = _CALL, ks(c), ws_bytes(c)
    call.entry, call.trans_a, call.trans_b, call.M, call.N, call.count = _ENTRY[c.entry], c.ta, c.tb, c.M, c.N, c.count
    call.has_ws, call.ws_bytes, call.mode = int(wsb is not None), wsb or 0, c.mode
    for i in range(4):
        live = i < len(lda)
        call.K[i] = K[i] if i < len(K) else 0
        call.lda[i], call.ldb[i], call.ldc[i], call.n_pad[i] = (lda[i], ldb[i], ldc[i], n_pad[i]) if live else (0, 0, 0, 0)
        call.base_a[i], call.base_b[i], call.base_lo[i] = (ba[i], bb[i], ba[i]) if live else (0, 0, 0)
    out = F_.GemmForm() if out is None else out
    _lib.check(_LIB().ggpm_gemm_form_query(ctypes.byref(call), ctypes.byref(out)), "gemm_form_query")
    return out


def reduce_form(entry, ta, tb, M, N, K, count, f):
    """the reduced form of a query result: (kernel, ta, tb, vecA, vecB, split, reduce, count, ragged M, N, K)"""
    if f.rc != OK:
        return ("refused", f.rc)
    kernel = F_.GEMM_KERNELS[f.kernel]
    tile = TILES.get(kernel)
    K = K if isinstance(K, (tuple, list)) else (K,)
    if not tile:          # a sequence of ggpm_gemm calls: each member has the form ggpm_gemm reports for it
        return (kernel, ta, tb, 0, 0, False, "none", count, False, False, False)
    rag = (M % tile[0] != 0, N % tile[1] != 0, any(k % tile[2] != 0 for k in K))
    return (kernel, ta, tb, f.vec_a, f.vec_b, f.splits > 1, F_.GEMM_REDUCES[f.reduce], count) + rag


def form_key(entry, red):
    """(entry, reduced form): a split-K group that does not split IS a ggpm_gemm_grouped call, a tn_bf16 call a group of one"""
    if entry == "grouped_splitk" and (len(red) < 7 or red[6] != "splitk_reduce_group") and red[0] != "refused":
        entry = "grouped"
    return (entry,) + red


def bits(c, s):
    return sum((v == "v") << i for i, v in enumerate(members(c, s)))


def expected(c):
    """the reduced form the table states for a case"""
    if c.rc != OK:
        return ("refused", c.rc)
    tile = TILES.get(c.kernel)
    K = ks(c) if c.entry in ("ksegments", "tall_grouped") else ks(c)[:1]
    if not tile:
        return (c.kernel, c.ta, c.tb, 0, 0, False, "none", c.count, False, False, False)
    rag = (c.M % tile[0] != 0, c.N % tile[1] != 0, any(k % tile[2] != 0 for k in K))
    return (c.kernel, c.ta, c.tb, bits(c, c.va), bits(c, c.vb), c.split, c.reduce, c.count) + rag


def reduced(c):
    K = ks(c) if c.entry in ("ksegments", "tall_grouped") else ks(c)[:1]
    return reduce_form(c.entry, c.ta, c.tb, c.M, c.N, K, c.count, query(c))


CASES = []


def case(name, entry, ta, tb, M, N, K, kernel, count=1, va="v", vb="v", n_pad=None, ldc_extra=3, ws="none", mode=0, split=False,
         reduce="none", rc=OK):
    join = lambda v: "".join(v) if isinstance(v, tuple) else v
    full = "%s-%s-%d%d-%dx%dx%s-c%d-%s.%s-%s-m%d" % (name, entry, ta, tb, M, N, "+".join(map(str, K)) if isinstance(K, tuple) else K,
                                                     count, join(va), join(vb), ws, mode)
    va, vb = join(va), join(vb)
    CASES.append(Case(full, entry, ta, tb, M, N, K, count, va, vb, n_pad, ldc_extra, ws, mode, kernel, split, reduce, rc))


TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
BOOL3 = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]

# ---- ggpm_gemm on the scalar 64 x 64 kernel: an operand that does not allow 16-byte loads -------------------------------------
for ta, tb in TRANS:
    for va, vb in (("l", "l"), ("v", "l"), ("l", "v")):          # neither legal, A only, B only
        for rm, rn, rk in BOOL3:
            case("scalar", "gemm", ta, tb, 64 + rm, 64 + rn, 32 + rk, "gemm_kernel", va=va, vb=vb, n_pad=64 + rn + 2 * rn)
    for off in "123":                                          # illegal by base alone (the column views W[:, 62:])
        case("scalar-base", "gemm", ta, tb, 65, 63, 33, "gemm_kernel", va=off, vb="v")
        case("scalar-base", "gemm", ta, tb, 63, 65, 31, "gemm_kernel", va="v", vb=off)
    case("scalar-one", "gemm", ta, tb, 1, 1, 1, "gemm_kernel", va="l", vb="l")
    case("scalar-edges", "gemm", ta, tb, 63, 1, 31, "gemm_kernel", va="l", vb="v")
    case("scalar-edges", "gemm", ta, tb, 1, 63, 1, "gemm_kernel", va="v", vb="l")
    # split-K on the scalar kernel: a workspace and K >= 2048
    for va, vb in (("l", "l"), ("v", "l"), ("l", "v")):
        for rm, rn, rk in BOOL3:
            case("scalar-splitk", "gemm", ta, tb, 64 + rm, 64 + rn, 2048 + rk, "gemm_kernel", va=va, vb=vb, ws="exact", split=True,
                 reduce="splitk_reduce")

# ---- gemm_small_v3: aligned, at most 300 tiles of 64 x 64 -------------------------------------------------------------------
for ta, tb in TRANS:
    for rm, rn, rk in BOOL3:
        case("v3", "gemm", ta, tb, 32 + rm, 32 + rn, 64 + rk, "gemm_small_v3", n_pad=32 + rn + 4 * rk)
    case("v3-one", "gemm", ta, tb, 1, 1, 1, "gemm_small_v3")
    case("v3-edges", "gemm", ta, tb, 31, 33, 63, "gemm_small_v3")
    case("v3-edges", "gemm", ta, tb, 33, 31, 129, "gemm_small_v3", n_pad=40)
case("v3-300-tiles", "gemm", 0, 1, 64 * 20, 64 * 15, 65, "gemm_small_v3")
case("v3-301-tiles", "gemm", 0, 1, 64 * 43, 64 * 7, 65, "gemm_kernel_v2")

# ---- gemm_kernel_v2: aligned, more than 300 tiles, the whole grid resident (<= 512 workgroups) ----------------------------------
for ta, tb in TRANS:
    for rm, rn, rk in BOOL3:
        case("v2", "gemm", ta, tb, 64 * 19 + rm, 64 * 16 + rn, 64 + rk, "gemm_kernel_v2", n_pad=64 * 16 + 4 * rn)
    for K in (63, 127, 128, 129):                              # odd and even counts of k-steps, the K-tail mask
        case("v2-steps", "gemm", ta, tb, 64 * 7 + 1, 64 * 43 + 1, K, "gemm_kernel_v2")
    # ... and beyond 512 workgroups the scalar kernel, with both operands vector-legal
    for rm, rn, rk in BOOL3:
        case("nonresident", "gemm", ta, tb, 64 * 33 - rm, 64 * 16 - rn, 32 + rk, "gemm_kernel")
case("resident-512", "gemm", 0, 1, 64 * 32, 64 * 16, 33, "gemm_kernel_v2")
case("resident-513", "gemm", 0, 1, 64 * 32, 64 * 16 + 1, 33, "gemm_kernel")      # 32 x 17 = 544 workgroups

# ---- plain split-K (choose_splits: K >= 2048, fewer than 512 tiles) with splitk_reduce --------------------------------------
for ta, tb in TRANS:
    for rm, rn, rk in BOOL3:
        # few tiles: tiles x splits <= 512 on gemm_kernel_v2; 100 tiles x 8 chunks = 800 workgroups on the scalar kernel
        case("v2-splitk", "gemm", ta, tb, 64 + rm, 64 + rn, 2048 + rk, "gemm_kernel_v2", ws="exact", split=True, reduce="splitk_reduce",
             n_pad=64 + 3 * rn)
        case("nonresident-splitk", "gemm", ta, tb, 640 - rm, 640 - rn, 2048 + rk, "gemm_kernel", ws="exact", split=True,
             reduce="splitk_reduce")
case("splitk-2047", "gemm", 0, 1, 65, 65, 2047, "gemm_small_v3", ws=1 << 20)
case("splitk-2048", "gemm", 0, 1, 65, 65, 2048, "gemm_kernel_v2", ws=1 << 20, split=True, reduce="splitk_reduce")
case("splitk-short-ws", "gemm", 0, 1, 65, 65, 2048, "gemm_small_v3", ws="short")
case("splitk-511-tiles", "gemm", 0, 1, 64 * 73, 64 * 7, 2048, "gemm_kernel", ws="full", split=True, reduce="splitk_reduce")
case("splitk-512-tiles", "gemm", 0, 1, 64 * 32, 64 * 16, 2048, "gemm_kernel_v2", ws=1 << 20)

# ---- tall contractions (ta = 1, tb = 0, aligned, K >= 6144, M, N >= 64, cover >= 0.8) ------------------------------------------
for rm, rn, rk in BOOL3:
    M, N = 160 - rm, 160 - rn
    case("tall-direct", "gemm", 1, 0, M, N, 6144 + rk, "gemm_tn_tall", ws="none", n_pad=N + rn)
    case("tall-underslab", "gemm", 1, 0, M, N, 6144 + rk, "gemm_tn_tall", ws="underslab")
    case("tall-slab", "gemm", 1, 0, M, N, 6144 + rk, "gemm_tn_tall_split", ws="slab", reduce="tall_reduce")
    case("tall-full", "gemm", 1, 0, M, N, 6144 + rk, "gemm_tn_tall_split", ws="full", split=True, reduce="tall_reduce", n_pad=160)
case("tall-K-6143", "gemm", 1, 0, 160, 160, 6143, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")
case("tall-K-tail-31", "gemm", 1, 0, 160, 160, 6144 + 31, "gemm_tn_tall_split", ws="full", split=True, reduce="tall_reduce")
case("tall-cover-0.8", "gemm", 1, 0, 160, 128, 6144, "gemm_tn_tall_split", ws="full", split=True, reduce="tall_reduce")
case("tall-cover-under", "gemm", 1, 0, 160, 127, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")
case("tall-M-63", "gemm", 1, 0, 63, 160, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")
case("tall-M-64", "gemm", 1, 0, 64, 64, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")      # cover 0.16
case("tall-M-64", "gemm", 1, 0, 64, 320, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")     # cover 0.4
case("tall-two-tiles", "gemm", 1, 0, 161, 255, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")  # cover 0.40
case("tall-two-tiles", "gemm", 1, 0, 150, 300, 6145, "gemm_tn_tall_split", ws="full", split=True, reduce="tall_reduce")
case("tall-two-tiles", "gemm", 1, 0, 300, 150, 6145, "gemm_tn_tall", ws="none")
case("tall-n-pad-max", "gemm", 1, 0, 150, 150, 6144, "gemm_tn_tall_split", ws="full", split=True, reduce="tall_reduce", n_pad=160)
case("tall-n-pad-past", "gemm", 1, 0, 150, 150, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce", n_pad=161)
case("tall-unaligned", "gemm", 1, 0, 160, 160, 6144, "gemm_kernel", va="l", ws="full", split=True, reduce="splitk_reduce")
for ta, tb in ((0, 0), (0, 1), (1, 1)):
    case("tall-other-transposes", "gemm", ta, tb, 160, 160, 6144, "gemm_kernel_v2", ws="full", split=True, reduce="splitk_reduce")

# ---- ggpm_gemm_tall_grouped ---------------------------------------------------------------------------------------------------
TALL_MODE = {0: "gemm_tn_tall_split", 1: "gemm_tn_tall_bf16<false>", 2: "gemm_tn_tall_bf16<true>"}
for mode in (0, 1, 2):
    for count in (1, 2, 3, 4):
        for rm, rn, rk in BOOL3:
            # unequal K: the chunk length is rounded up per member, so member 1 gets fewer chunks than the group's splits and
            # writes zero slabs for the rest
            K = tuple(k + d * rk for k, d in zip((6144, 6144 + 32, 12288, 6144 + 64), (1, 31, 1, 33)))[:count]
            M, N = 160 - rm, 160 - rn
            if count == 1 and mode == 0:
                if (rm, rn, rk) == (1, 0, 0):
                    case("tall-group-of-one", "tall_grouped", 1, 0, M, N, K, "sequence", count=1, ws="full", mode=0)
                continue
            case("tall-group", "tall_grouped", 1, 0, M, N, K, TALL_MODE[mode], count=count, ws="full", mode=mode, split=True,
                 reduce="tall_reduce", n_pad=160)
            # one chunk per member (a workspace of one slab each): nothing to be unequal about, the smallest K of the form
            K1 = tuple(k + d * rk for k, d in zip((6144, 6144 + 32, 6144 + 64, 6144 + 96), (1, 31, 1, 33)))[:count]
            case("tall-group-one-chunk", "tall_grouped", 1, 0, M, N, K1, TALL_MODE[mode], count=count, ws="slab", mode=mode,
                 reduce="tall_reduce", n_pad=(N, 160, N, N + rn)[:count])
    # a member that does not qualify (K below 6144): fp32 operands run as a sequence, bf16 operands in memory are refused
    if mode < 2:
        for count in (2, 3, 4):
            case("tall-group-unqualified", "tall_grouped", 1, 0, 160, 160, (6144, 6143, 6144, 6144)[:count], "sequence", count=count,
                 ws="full", mode=mode)
        case("tall-group-no-ws", "tall_grouped", 1, 0, 160, 160, (6144, 6144), "sequence", count=2, ws="none", mode=mode)
    else:
        case("tall-group-unqualified", "tall_grouped", 1, 0, 160, 160, (6144, 6143), "none", count=2, ws="full", mode=2,
             rc=ERR_UNSUPPORTED)
case("tn-bf16", "tn_bf16", 1, 0, 159, 159, 6145, "gemm_tn_tall_bf16<false>", ws="full", split=True, reduce="tall_reduce")
case("tn-bf16-short-K", "tn_bf16", 1, 0, 160, 160, 6143, "sequence", ws="full")

# ---- ggpm_gemm_grouped / _splitk / _masked ------------------------------------------------------------------------------------
for ta, tb in TRANS:
    for count in (2, 3, 4):
        for rm, rn, rk in BOOL3:
            case("group-v3", "grouped", ta, tb, 32 + rm, 32 + rn, 64 + rk, "gemm_small_v3", count=count,
                 n_pad=(32 + rn, 36, 40, 33)[:count])
            case("group-v2", "grouped", ta, tb, 64 * 11 + rm, 64 * 14 + rn, 64 + rk, "gemm_group_v2", count=count)
            for va, vb in (("l", "l"), ("v", "l"), ("l", "v")):       # every member on scalar loads, for one reason
                case("group-scalar", "grouped", ta, tb, 64 + rm, 64 + rn, 32 + rk, "gemm_kernel_group", count=count, va=va, vb=vb,
                     n_pad=(64 + rn, 70, 65 + rn, 66)[:count])
        # ... and for a different reason each (leading dimension, base)
        case("group-scalar-reasons", "grouped", ta, tb, 65, 63, 33, "gemm_kernel_group", count=count, va=("l", "v", "2", "l")[:count],
             vb=("v", "l", "v", "3")[:count])
        case("group-mixed", "grouped", ta, tb, 65, 63, 33, "sequence", count=count, va=("v", "l", "v", "v")[:count])
    case("group-of-one", "grouped", ta, tb, 33, 33, 65, "sequence", count=1)
    for count in (1, 2, 3, 4):
        for rm, rn, rk in BOOL3:          # K in chunks: few tiles, K / 256 >= 2 chunks
            case("group-splitk", "grouped_splitk", ta, tb, 32 + rm, 32 + rn, 512 + rk, "gemm_small_v3", count=count, ws="exact",
                 split=True, reduce="splitk_reduce_group", n_pad=(32 + rn, 36, 32 + rn, 40)[:count])
for count in (1, 2, 3, 4):
    case("group-splitk-last-chunk-of-one", "grouped_splitk", 1, 0, 33, 31, 1281, "gemm_small_v3", count=count, ws="exact", split=True,
         reduce="splitk_reduce_group")
    case("group-splitk-too-short", "grouped_splitk", 1, 0, 33, 31, 511, "gemm_small_v3" if count > 1 else "sequence", count=count,
         ws=1 << 20)
    case("group-masked", "grouped_masked", 0, 1, 33, 31, 65, "gemm_small_v3", count=count)
case("group-splitk-short-ws", "grouped_splitk", 1, 0, 33, 31, 513, "gemm_small_v3", count=2, ws=1024)
case("group-masked-300-tiles", "grouped_masked", 0, 1, 64 * 10, 64 * 10, 33, "gemm_small_v3", count=3)
case("group-masked-304-tiles", "grouped_masked", 0, 1, 64 * 19, 64 * 4, 33, "none", count=4, rc=ERR_UNSUPPORTED)
case("group-masked-unaligned", "grouped_masked", 0, 1, 33, 31, 65, "none", count=2, va="vl", rc=ERR_UNSUPPORTED)

# ---- ggpm_gemm_ksegments --------------------------------------------------------------------------------------------------------
SEG_K = (64, 1, 63, 65)
for tb in (0, 1):
    for nseg in (2, 3, 4):
        for rm, rn, rk in BOOL3:
            Kr = SEG_K[:nseg] if rk else (64,) * nseg
            case("segs-v3", "ksegments", 0, tb, 32 + rm, 32 + rn, Kr, "gemm_small_v3", count=nseg)
            case("segs-v2", "ksegments", 0, tb, 64 * 19 + rm, 64 * 16 + rn, Kr, "gemm_kernel_v2", count=nseg)
            Ks = tuple(32 if k == 64 else k for k in Kr)
            for va, vb in (("l", "l"), ("v", "l"), ("l", "v")):
                case("segs-scalar", "ksegments", 0, tb, 64 + rm, 64 + rn, Ks, "gemm_kernel_segs", count=nseg, va=va, vb=vb,
                     n_pad=64 + rn + 2)
        case("segs-scalar-reasons", "ksegments", 0, tb, 65, 63, (32, 1, 63, 65)[:nseg], "gemm_kernel_segs", count=nseg,
             va=("l", "v", "2", "l")[:nseg], vb=("v", "l", "v", "3")[:nseg])
        case("segs-mixed", "ksegments", 0, tb, 65, 63, (32, 1, 63, 65)[:nseg], "sequence", count=nseg, va=("l", "v", "v", "v")[:nseg])
    case("segs-of-one", "ksegments", 0, tb, 33, 31, (65,), "sequence", count=1)

# ---- ggpm_gemm_tn_pair_grouped ------------------------------------------------------------------------------------------------
for count in (2, 3, 4):
    for rm, rn, rk in BOOL3:
        case("pairs", "pair_grouped", 1, 0, 32 + rm, 32 + rn, 64 + rk, "gemm_small_v3", count=count)
    case("pairs-too-many-tiles", "pair_grouped", 1, 0, 64 * 11, 64 * 14, 65, "sequence", count=count)
case("pairs", "pair_grouped", 1, 0, 33, 31, 65, "gemm_small_v3", count=1)

# ---- refusals: GGPM_ERR_ARG of the shape checks (the null operands are tests/test_gpu_gemm_forms.py's) ---------------------------
REFUSALS = [
    Case("refuse-n_pad-below-N", "gemm", 0, 1, 33, 31, 65, 1, "v", "v", 30, 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-n_pad-above-ldc", "gemm", 0, 1, 33, 31, 65, 1, "v", "v", 32, -2, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-count-0", "grouped", 0, 1, 33, 31, 65, 0, "v", "v", None, 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-count-5", "grouped", 0, 1, 33, 31, 65, 5, "v", "v", None, 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-group-n_pad-below-N", "grouped", 0, 1, 33, 31, 65, 2, "v", "v", (31, 30), 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-masked-n_pad-above-ldc", "grouped_masked", 0, 1, 33, 31, 65, 2, "v", "v", (31, 33), -1, "none", 0, "none", False,
         "none", ERR_ARG),
    Case("refuse-splitk-count-5", "grouped_splitk", 1, 0, 33, 31, 513, 5, "v", "v", None, 3, "exact", 0, "none", False, "none", ERR_ARG),
    Case("refuse-segs-n_pad-below-N", "ksegments", 0, 1, 33, 31, (65, 64), 2, "v", "v", 30, 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-segs-nseg-5", "ksegments", 0, 1, 33, 31, (65,) * 5, 5, "v", "v", None, 3, "none", 0, "none", False, "none", ERR_ARG),
    Case("refuse-tall-count-5", "tall_grouped", 1, 0, 160, 160, (6144,) * 5, 5, "v", "v", None, 3, "full", 0, "none", False, "none", ERR_ARG),
    Case("refuse-pairs-count-0", "pair_grouped", 1, 0, 33, 31, 65, 0, "v", "v", None, 3, "none", 0, "none", False, "none", ERR_ARG),
]

# ---- column sums (no form query: the three launch forms by row count and dtype) ---------------------------------------------------
COLSUM = [(M, N, ld_extra, bf16) for bf16 in (0, 1) for M, N, ld_extra in
          [(1, 1, 0), (2048, 63, 1), (2049, 64, 0), (32768, 65, 3), (32769, 1, 7), (40001, 300, 4), (2049, 300, 0), (1, 65, 2)]]


def case_id(c):
    return c.name


NAMED = ["scalar", "scalar-base", "scalar-one", "scalar-edges", "scalar-splitk", "v3", "v3-one", "v3-edges", "v3-300-tiles", "v3-301-tiles",
         "v2", "v2-steps", "nonresident", "resident-512", "resident-513", "v2-splitk", "nonresident-splitk", "splitk-2047",
         "splitk-2048", "splitk-short-ws", "splitk-511-tiles", "splitk-512-tiles", "tall-direct", "tall-underslab", "tall-slab",
         "tall-full", "tall-K-6143", "tall-K-tail-31", "tall-cover-0.8", "tall-cover-under", "tall-M-63", "tall-M-64",
         "tall-two-tiles", "tall-n-pad-max", "tall-n-pad-past", "tall-group", "tall-group-one-chunk", "tall-group-unqualified",
         "tall-group-no-ws", "tn-bf16", "group-v3", "group-v2", "group-scalar", "group-mixed", "group-of-one", "group-splitk",
         "group-splitk-last-chunk-of-one", "group-masked", "group-masked-300-tiles", "group-masked-304-tiles", "segs-v3",
         "segs-v2", "segs-scalar", "segs-mixed", "segs-of-one", "pairs", "pairs-too-many-tiles"]
