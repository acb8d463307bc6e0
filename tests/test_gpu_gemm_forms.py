"""GPU: every case of tests/gemm_form_cases.py against the fp64 product of the same operands, with poisoned padding.

Each case first asserts with ggpm_gemm_form_query that the call takes the kernel the table states (tests/
test_gemm_forms_cpu.py holds the table against the lattice of reachable forms), then runs it on operands that are views
inside NaN-filled allocations: NaN rows before and after, NaN in every column between the logical width and the leading
dimension.  C and its guard rows hold a sentinel, the workspace is followed by guard words.  Two bars:
  * the project's max-norm bars: 2e-6 (K <= 5000) / 5e-6 for ggpm_gemm, 3e-6 grouped and segmented, 2e-6 for bf16 operands
    against the fp64 product of the rounded operands;
  * componentwise, |got - ref| / (sum_k |a_mk| |b_kn| + |bias_n| + |addend_mn|), at most 3x the worst value of a strict
    k-ordered fp32 accumulation chain (numpy float32, one accumulator per output, the same operands, a fixed sample of
    4096 outputs) plus 1e-7.  The factor 3 covers the maximum over a sample against the whole matrix and FMA against
    separate rounding.  profiles/gemm_forms.txt records what each form measured.
Operand rows along k are scaled by 1e-3 ... 1e3 and the other operand by the inverse, so the outputs keep ordinary
magnitudes while a dropped low-order term or a misplaced row shows.  Every case runs twice: identical bits."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gemm_form_cases as C
from ggpm_amd import _lib
from ggpm_amd import functional as F_

pytestmark = pytest.mark.gpu

SENTINEL, WS_GUARD = -777.25, 12345.0
SAMPLE = 4096


class GemmEpilogue(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_gemm_epilogue"""
    _fields_ = [("addend", ctypes.c_void_p), ("ld_addend", ctypes.c_int), ("mask_y", ctypes.c_void_p),
                ("mask_out", ctypes.c_void_p), ("ld_mask", ctypes.c_int), ("mask_act", ctypes.c_int),
                ("mask_zero_row0", ctypes.c_int)]


def _dev():
    return torch.device("cuda:0")


def _poisoned(values, ld, off, dtype=torch.float32):
    """`values` [rows, width] as a [rows, ld] view, `off` elements into a NaN-filled allocation with four NaN rows before
    and after it; the columns width .. ld - 1 stay NaN.  -> (allocation, view)"""
    rows, width = values.shape
    buf = torch.full(((rows + 8) * ld + 8,), float("nan"), dtype=dtype, device=_dev())
    view = buf[4 * ld + off: 4 * ld + off + rows * ld].view(rows, ld)
    view[:, :width] = torch.from_numpy(values).to(_dev()).to(dtype)
    return buf, view


def _c_buffer(M, ldc, init=None):
    """C [M, ldc] inside a sentinel-filled allocation with four guard rows before and after -> (allocation, view)"""
    buf = torch.full(((M + 8) * ldc,), SENTINEL, dtype=torch.float32, device=_dev())
    view = buf[4 * ldc: (4 + M) * ldc].view(M, ldc)
    if init is not None:
        view[:, :init.shape[1]] = torch.from_numpy(init).to(_dev())
    return buf, view


def _workspace(nbytes):
    if nbytes is None:
        return None, 0
    words = -(-nbytes // 4)
    ws = torch.full((words + 64,), WS_GUARD, dtype=torch.float32, device=_dev())
    return ws, words


def _chain32(a, b, mi, ni):
    """strict k-ordered fp32 accumulation, one accumulator per sampled output (mi[j], ni[j]): a [M, K], b [K, N] float32"""
    out = np.empty(len(mi), dtype=np.float32)
    for lo in range(0, len(mi), 512):
        p = a[mi[lo:lo + 512], :] * b[:, ni[lo:lo + 512]].T              # float32 products, rounded one by one
        out[lo:lo + 512] = np.add.accumulate(p, axis=1, dtype=np.float32)[:, -1]
    return out


class Member:
    """one product of a case: host operands (as the kernel sees them after any bf16 rounding), epilogue, device buffers"""


def _epilogue_flags(c, idx, i):
    h = (idx * 7 + i * 3) & 15
    if c.entry in ("pair_grouped", "tn_bf16") or c.rc != C.OK:
        return 0, 0, 0, 0
    return h & 1, h >> 1 & 1, h >> 2 & 1, h >> 3 & 1      # bias, accumulate, relu, zero_row0


def _segments(c, i):
    """-> [(A is k-major?, B is k-major?, K)] of member i: one product per K segment"""
    K = C.ks(c)
    if c.entry == "ksegments":
        return [(False, not c.tb, k) for k in K]
    if c.entry == "pair_grouped":
        return [(True, True, K[0])] * 2
    return [(bool(c.ta), not c.tb, K[i] if c.entry == "tall_grouped" else K[0])]


def _build(c, idx):
    """device operands and the fp64 / fp32-chain references of every member"""
    rs = np.random.RandomState(idx * 13 + 5)
    lda, ldb, ldc, n_pad, _, _ = C.geometry(c)
    in16 = c.mode == 2
    rounded = c.mode in (1, 2) or c.entry == "tn_bf16"
    dt = torch.bfloat16 if in16 else torch.float32
    n_members = 1 if c.entry == "ksegments" else c.count
    members, keep = [], []
    for i in range(n_members):
        m = Member()
        m.A, m.B = [], []
        ref = np.zeros((c.M, c.N)); den = np.zeros((c.M, c.N)); a_cat, b_cat = [], []
        for s, (a_kmajor, b_kmajor, k) in enumerate(_segments(c, i)):
            j = s if c.entry == "ksegments" else i
            scale = np.exp(rs.uniform(math.log(1e-3), math.log(1e3), size=k)).astype(np.float32)
            a = rs.standard_normal((c.M, k)).astype(np.float32) * scale               # A'(m, k)
            b = rs.standard_normal((k, c.N)).astype(np.float32) / scale[:, None]      # B'(k, n)
            if c.entry == "pair_grouped":
                if s == 0:
                    pair_b = b
                else:                      # lo: the rounding errors of a sum, far below hi; the same B
                    a, b = a * np.float32(1e-5), pair_b
            if rounded:
                a = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
                b = torch.from_numpy(b).to(torch.bfloat16).float().numpy()
            va, vb = C.members(c, c.va)[j], C.members(c, c.vb)[j]
            la, lb = (lda[0], ldb[0]) if c.entry == "pair_grouped" else (lda[j], ldb[j])
            if not (c.entry == "pair_grouped" and s == 1):
                bufb, vB = _poisoned(np.ascontiguousarray(b if b_kmajor else b.T), lb, C.off_of(vb), dt)
            bufa, vA = _poisoned(np.ascontiguousarray(a.T if a_kmajor else a), la, C.off_of(va), dt)
            keep += [bufa, bufb]
            m.A.append(vA); m.B.append(vB)
            ref += a.astype(np.float64) @ b.astype(np.float64)
            den += np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
            a_cat.append(a); b_cat.append(b)
        m.bias_on, m.acc, m.relu, m.zero_row0 = _epilogue_flags(c, idx, i)
        m.bias = rs.standard_normal(c.N).astype(np.float32) if m.bias_on else None
        m.c0 = rs.standard_normal((c.M, c.N)).astype(np.float32) if m.acc else None
        m.ldc, m.n_pad = ldc[i], n_pad[i]
        # references: fp64, and the fp32 chain on a fixed sample
        nout = c.M * c.N
        pick = np.arange(nout) if nout <= SAMPLE else np.sort(rs.choice(nout, SAMPLE, replace=False))
        mi, ni = pick // c.N, pick % c.N
        chain = _chain32(np.concatenate(a_cat, axis=1), np.concatenate(b_cat, axis=0), mi, ni)
        if m.bias is not None:
            ref += m.bias; den += np.abs(m.bias); chain = chain + m.bias[ni]
        if m.c0 is not None:
            ref += m.c0; den += np.abs(m.c0); chain = chain + m.c0[mi, ni]
        if m.relu:
            ref = np.maximum(ref, 0.0); chain = np.maximum(chain, np.float32(0))
        if m.zero_row0:
            ref[0] = 0.0; chain = np.where(mi == 0, np.float32(0), chain)
        m.ref, m.den = ref, np.maximum(den, 1e-300)
        m.chain_worst = float((np.abs(chain.astype(np.float64) - ref[mi, ni]) / m.den[mi, ni]).max())
        m.bias_dev = None if m.bias is None else torch.from_numpy(m.bias).to(_dev())
        members.append(m)
    return members, keep


def _problems(members):
    arr = (F_.GemmProblem * len(members))()
    for i, m in enumerate(members):
        arr[i] = F_.GemmProblem(m.A[0].data_ptr(), m.A[0].stride(0), m.B[0].data_ptr(), m.B[0].stride(0), m.C.data_ptr(), m.ldc,
                                m.n_pad, F_._p(m.bias_dev), m.acc, F_.ACT_RELU if m.relu else F_.ACT_NONE, m.zero_row0)
    return arr


def _call(c, members, ws, nbytes):
    """the case's entry point on the members' current C buffers -> return code"""
    lib, s, m0 = _lib.load(build_if_missing=False), F_._stream(), members[0]
    K = C.ks(c)
    act = lambda m: F_.ACT_RELU if m.relu else F_.ACT_NONE
    if c.entry == "gemm":
        return lib.ggpm_gemm(c.ta, c.tb, c.M, c.N, K[0], m0.A[0].data_ptr(), m0.A[0].stride(0), m0.B[0].data_ptr(),
                             m0.B[0].stride(0), m0.C.data_ptr(), m0.ldc, m0.n_pad, F_._p(m0.bias_dev), m0.acc, act(m0),
                             m0.zero_row0, F_._p(ws), nbytes or 0, s)
    if c.entry == "grouped":
        return lib.ggpm_gemm_grouped(c.ta, c.tb, c.M, c.N, K[0], c.count, _problems(members), s)
    if c.entry == "grouped_splitk":
        return lib.ggpm_gemm_grouped_splitk(c.ta, c.tb, c.M, c.N, K[0], c.count, _problems(members), F_._p(ws), nbytes or 0, s)
    if c.entry == "grouped_masked":
        ep = (GemmEpilogue * c.count)()
        for i, m in enumerate(members):
            ep[i] = GemmEpilogue(m.addend.data_ptr() if m.acc else None, c.N + 1, m.mask_y.data_ptr(), m.mask_out.data_ptr(),
                                 c.N + 2, F_.ACT_RELU, int(i == 1))
        return lib.ggpm_gemm_grouped_masked(c.ta, c.tb, c.M, c.N, K[0], c.count, _problems(members), ep, s)
    if c.entry == "ksegments":
        n = c.count
        vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
        return lib.ggpm_gemm_ksegments(c.tb, c.M, c.N, n, vp(*[a.data_ptr() for a in m0.A]), ci(*[a.stride(0) for a in m0.A]),
                                       vp(*[b.data_ptr() for b in m0.B]), ci(*[b.stride(0) for b in m0.B]), ci(*K),
                                       m0.C.data_ptr(), m0.ldc, m0.n_pad, F_._p(m0.bias_dev), m0.acc, act(m0), m0.zero_row0, s)
    if c.entry == "tall_grouped":
        return lib.ggpm_gemm_tn_tall_grouped(c.M, c.N, c.count, _problems(members), (ctypes.c_int * c.count)(*K), F_._p(ws),
                                             nbytes or 0, c.mode, s)
    if c.entry == "tn_bf16":
        return lib.ggpm_gemm_tn_bf16(c.M, c.N, K[0], m0.A[0].data_ptr(), m0.A[0].stride(0), m0.B[0].data_ptr(), m0.B[0].stride(0),
                                     m0.C.data_ptr(), m0.ldc, F_._p(ws), nbytes or 0, s)
    assert c.entry == "pair_grouped"
    arr = (F_.PairProblem * max(c.count, len(members)))()
    for i, m in enumerate(members):
        arr[i] = F_.PairProblem(m.A[0].data_ptr(), m.A[1].data_ptr(), m.B[0].data_ptr(), m.C.data_ptr(), m.ldc)
    return lib.ggpm_gemm_tn_pair_grouped_c(c.M, c.N, K[0], m0.A[0].stride(0), c.count, arr, s)


def _fresh_outputs(c, members):
    for m in members:
        m.Cbuf, m.C = _c_buffer(c.M, m.ldc, None if c.entry == "grouped_masked" else m.c0)
        if c.entry == "grouped_masked":        # accumulate adds to `addend`, C is overwritten; a second output mask_out
            m.addend = _poisoned(m.c0, c.N + 1, 0)[1] if m.acc else None
            m.mask_y_host = np.random.RandomState(c.M + c.N).standard_normal((c.M, c.N)).astype(np.float32)
            m.mask_y = _poisoned(m.mask_y_host, c.N + 2, 0)[1]
            m.mask_buf, m.mask_out = _c_buffer(c.M, c.N + 2)


def _max_bar(c):
    """The project's max-norm bars.  A product on bf16 operands is held at 2e-6 against the rounded operands; a product
    over more than 5000 terms at 5e-6 whichever entry point issues it (the strict fp32 chain itself measures 3e-6 to 5e-6
    at K = 12288 on these operands); below that 2e-6 for ggpm_gemm and 3e-6 for the grouped and segmented launches.  A
    sequence of ggpm_gemm calls is ggpm_gemm's fp32 kernels whatever the mode asked for."""
    K = sum(C.ks(c)) if c.entry == "ksegments" else max(C.ks(c))
    if (c.mode in (1, 2) or c.entry == "tn_bf16") and c.kernel != "sequence":
        return 2e-6
    if K > 5000:
        return 5e-6
    return 2e-6 if c.entry == "gemm" else 3e-6


def _same_pointer_bits(c, members):
    lda, ldb, ldc, n_pad, ba, bb = C.geometry(c)
    for i, m in enumerate(members):
        for s in range(len(m.A)):
            j = s if c.entry == "ksegments" else i
            assert m.A[s].data_ptr() & 15 == ba[j] and m.B[s].data_ptr() & 15 == bb[j], (c.name, i, s)


def _run(c, idx):
    assert C.reduced(c) == C.expected(c), (c.name, C.reduced(c), C.expected(c))        # the kernel the table says
    members, keep = _build(c, idx)
    _same_pointer_bits(c, members)
    nbytes = C.ws_bytes(c)
    results = []
    for attempt in range(2):
        _fresh_outputs(c, members)
        ws, words = _workspace(nbytes)
        rc = _call(c, members, ws, nbytes)
        assert rc == c.rc, (c.name, rc)
        torch.cuda.synchronize()
        if ws is not None:
            assert bool((ws[words:] == WS_GUARD).all()), c.name + ": wrote behind the workspace"
        results.append([m.Cbuf.clone() for m in members] + ([m.mask_buf.clone() for m in members] if c.entry == "grouped_masked" else []))
    for x, y in zip(*results):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), c.name + ": two runs differ"
    worst = (0.0, 0.0, 0.0)
    for i, m in enumerate(members):
        full = m.Cbuf.view(c.M + 8, m.ldc).cpu().numpy()
        got = full[4:4 + c.M]
        sent = np.float32(SENTINEL)
        assert (full[:4] == sent).all() and (full[4 + c.M:] == sent).all(), c.name + ": guard rows of C written"
        assert (got[:, m.n_pad:] == sent).all(), c.name + ": columns n_pad .. ldc written"
        assert (got[:, c.N:m.n_pad] == 0).all(), c.name + ": columns N .. n_pad not zero"
        out = got[:, :c.N].astype(np.float64)
        assert np.isfinite(out).all(), c.name + ": a poisoned pad element reached the output"
        err_max = float(np.abs(out - m.ref).max() / max(np.abs(m.ref).max(), 1e-12))
        err_cw = float((np.abs(out - m.ref) / m.den).max())
        bar_cw = 3.0 * m.chain_worst + 1e-7
        print("GEMMFORM %s member %d form %r max-norm %.3e (bar %.0e) componentwise %.3e chain %.3e bar %.3e"
              % (c.name, i, C.form_key(c.entry, C.expected(c)), err_max, _max_bar(c), err_cw, m.chain_worst, bar_cw))
        worst = max(worst, (err_cw / bar_cw, err_max, err_cw))
        assert err_max < _max_bar(c), (c.name, i, err_max)
        assert err_cw <= bar_cw, (c.name, i, err_cw, m.chain_worst, bar_cw)
        if c.entry == "grouped_masked":
            mo = m.mask_buf.view(c.M + 8, c.N + 2).cpu().numpy()
            want = got[:, :c.N] * (m.mask_y_host > 0)
            if i == 1:
                want[0] = 0
            assert np.array_equal(mo[4:4 + c.M, :c.N], want) and (mo[:4] == sent).all() and (mo[4 + c.M:] == sent).all() \
                and (mo[4:4 + c.M, c.N:] == sent).all(), c.name + ": mask_out"
    return members


def _refused(c, live, idx):
    """the refused call `c` on the operands of the valid call `live` (c itself where only the form is refused): the
    return code the query predicts, nothing written"""
    assert C.reduced(c) == C.expected(c)
    members, _ = _build(live, idx)
    _fresh_outputs(live, members)
    ws, _words = _workspace(C.ws_bytes(live))
    assert _call(c, members, ws, C.ws_bytes(live)) == c.rc, c.name
    torch.cuda.synchronize()
    for m in members:
        assert bool((m.Cbuf == SENTINEL).all()), c.name


CASE_IDS = [c.name for c in C.CASES]


@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=CASE_IDS)
def test_gemm_form(idx):
    c = C.CASES[idx]
    if c.rc != C.OK:           # a refusal: nothing launched, the destination untouched
        _refused(c, c, idx)
        return
    members = _run(c, idx)
    lib = _lib.load(build_if_missing=False)
    if c.kernel in ("gemm_kernel_segs", "gemm_kernel_group"):
        # the claims of csrc/gemm.hip: the segment chain in one launch rounds where the sequence of ggpm_gemm calls it
        # replaces rounds; the group launch computes the same tiles as its members run alone
        m0 = members[0]
        one = [m.Cbuf.clone() for m in members]
        _fresh_outputs(c, members)
        K = C.ks(c)
        for i in range(c.count):
            if c.kernel == "gemm_kernel_segs":
                last = i == c.count - 1
                rc = lib.ggpm_gemm(0, c.tb, c.M, c.N, K[i], m0.A[i].data_ptr(), m0.A[i].stride(0), m0.B[i].data_ptr(),
                                   m0.B[i].stride(0), m0.C.data_ptr(), m0.ldc, m0.n_pad if i == 0 else c.N,
                                   F_._p(m0.bias_dev) if i == 0 else None, m0.acc if i == 0 else 1,
                                   F_.ACT_RELU if last and m0.relu else F_.ACT_NONE, m0.zero_row0 if last else 0, None, 0, F_._stream())
            else:
                m = members[i]
                rc = lib.ggpm_gemm(c.ta, c.tb, c.M, c.N, K[0], m.A[0].data_ptr(), m.A[0].stride(0), m.B[0].data_ptr(), m.B[0].stride(0),
                                   m.C.data_ptr(), m.ldc, m.n_pad, F_._p(m.bias_dev), m.acc, F_.ACT_RELU if m.relu else F_.ACT_NONE,
                                   m.zero_row0, None, 0, F_._stream())
            assert rc == 0
        torch.cuda.synchronize()
        for x, m in zip(one, members):
            assert torch.equal(x.view(torch.int32), m.Cbuf.view(torch.int32)), c.name + ": not the bits of the separate calls"


@pytest.mark.parametrize("idx", range(len(C.REFUSALS)), ids=[c.name for c in C.REFUSALS])
def test_shape_refusals_launch_nothing(idx):
    """GGPM_ERR_ARG of the shape checks: the return code the query predicts, and C untouched"""
    c = C.REFUSALS[idx]
    assert C.reduced(c) == ("refused", C.ERR_ARG)
    _refused(c, c._replace(count=min(max(c.count, 1), 4), K=C.ks(c)[:4] if isinstance(c.K, tuple) else c.K), idx)


def test_null_operands_and_short_addends_are_refused():
    lib, s = _lib.load(build_if_missing=False), F_._stream()
    c = C.Case("null", "grouped", 0, 1, 33, 31, 65, 2, "v", "v", None, 3, "none", 0, "gemm_small_v3", False, "none", C.OK)
    members, _ = _build(c, 1)
    _fresh_outputs(c, members)
    m = members[0]
    before = [x.Cbuf.clone() for x in members]
    a, b, cc, lda, ldb = m.A[0].data_ptr(), m.B[0].data_ptr(), m.C.data_ptr(), m.A[0].stride(0), m.B[0].stride(0)
    for pa, pb, pc in ((None, b, cc), (a, None, cc), (a, b, None)):
        assert lib.ggpm_gemm(0, 1, 33, 31, 65, pa, lda, pb, ldb, pc, m.ldc, 31, None, 0, 0, 0, None, 0, s) == C.ERR_ARG
    for bad in ("A", "B", "C"):
        arr = _problems(members)
        setattr(arr[1], bad, None)
        assert lib.ggpm_gemm_grouped(0, 1, 33, 31, 65, 2, arr, s) == C.ERR_ARG
        ep = (GemmEpilogue * 2)()
        assert lib.ggpm_gemm_grouped_masked(0, 1, 33, 31, 65, 2, arr, ep, s) == C.ERR_ARG
    assert lib.ggpm_gemm_grouped(0, 1, 33, 31, 65, 2, None, s) == C.ERR_ARG
    ep = (GemmEpilogue * 2)()
    ep[0] = GemmEpilogue(m.C.data_ptr(), 30, None, None, 0, 0, 0)                      # ld_addend < N
    assert lib.ggpm_gemm_grouped_masked(0, 1, 33, 31, 65, 2, _problems(members), ep, s) == C.ERR_ARG
    ep[0] = GemmEpilogue(None, 0, None, m.C.data_ptr(), 31, 0, 0)                      # mask_out without mask_y
    assert lib.ggpm_gemm_grouped_masked(0, 1, 33, 31, 65, 2, _problems(members), ep, s) == C.ERR_ARG
    assert lib.ggpm_gemm_grouped_masked(0, 1, 33, 31, 65, 2, _problems(members), None, s) == C.ERR_ARG
    assert lib.ggpm_gemm_tn_tall_grouped(160, 160, 2, None, None, None, 0, 0, s) == C.ERR_ARG
    assert lib.ggpm_gemm_tn_tall_grouped(160, 160, 2, _problems(members), (ctypes.c_int * 2)(6144, 6144), None, 0, 3, s) == C.ERR_ARG
    assert lib.ggpm_gemm_tn_pair_grouped_c(33, 31, 65, 30, 2, (F_.PairProblem * 2)(), s) == C.ERR_ARG       # ld < M
    assert lib.ggpm_gemm_tn_pair_grouped_c(33, 31, 65, 36, 2, (F_.PairProblem * 2)(), s) == C.ERR_ARG       # null operands
    assert lib.ggpm_colsum_dtype(None, 4, 3, 3, cc, cc, 0, s) == C.ERR_ARG
    assert lib.ggpm_gemm_tn_bf16(160, 160, 6144, a, lda, b, ldb, cc, 159, cc, 1 << 20, s) == C.ERR_ARG       # ldc < N
    torch.cuda.synchronize()
    for m, was in zip(members, before):
        assert torch.equal(m.Cbuf.view(torch.int32), was.view(torch.int32))


@pytest.mark.parametrize("M,N,ld_extra,bf16", C.COLSUM)
def test_colsum_forms(M, N, ld_extra, bf16):
    """ggpm_colsum_dtype on the one-launch form (M <= 2048, fp32), the two-stage form, and past its 256-chunk cap
    (M > 32768), fp32 and bf16 input, lda > N with NaN pad columns"""
    lib = _lib.load(build_if_missing=False)
    rs = np.random.RandomState(M + N)
    a = (rs.standard_normal((M, N)) * np.exp(rs.uniform(math.log(1e-3), math.log(1e3), size=(M, 1)))).astype(np.float32)
    if bf16:
        a = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    buf, view = _poisoned(a, N + ld_extra, 0, torch.bfloat16 if bf16 else torch.float32)
    results = []
    for attempt in range(2):
        out = torch.full((N + 8,), SENTINEL, device=_dev())
        ws = torch.full((256 * N + 64,), WS_GUARD, device=_dev())
        assert lib.ggpm_colsum_dtype(view.data_ptr(), N + ld_extra, M, N, out.data_ptr(), ws.data_ptr(), bf16, F_._stream()) == 0
        torch.cuda.synchronize()
        assert bool((ws[256 * N:] == WS_GUARD).all()) and bool((out[N:] == SENTINEL).all())
        results.append(out)
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))
    got = results[0][:N].cpu().numpy().astype(np.float64)
    ref, den = a.astype(np.float64).sum(0), np.abs(a).astype(np.float64).sum(0)
    chain = np.add.accumulate(a.T, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    chain_worst = float((np.abs(chain - ref) / den).max())
    err_max, err_cw = float(np.abs(got - ref).max() / np.abs(ref).max()), float((np.abs(got - ref) / den).max())
    print("GEMMFORM colsum-%dx%d-ld+%d-bf16=%d member 0 form ('colsum', %d, %s) max-norm %.3e (bar %.0e) componentwise %.3e chain %.3e "
          "bar %.3e" % (M, N, ld_extra, bf16, bf16, "one" if M <= 2048 and not bf16 else "two-stage" if M <= 32768 else "capped",
                        err_max, math.inf, err_cw, chain_worst, 3 * chain_worst + 1e-7))     # (no max-norm bar: a sum that cancels)
    assert np.isfinite(got).all() and err_cw <= 3 * chain_worst + 1e-7, (err_cw, chain_worst)


def test_linear_wgrads_batch_is_the_separate_calls_bit_for_bit():
    """ggpm_linear_wgrads_batch: count 0; items with and without db; an item whose workspace need exceeds ws_bytes (runs
    unsplit); ws == NULL -- each time the bits of ggpm_gemm(1, 0, N, K, M, ...) + ggpm_colsum under the same workspace rule"""
    lib, s = _lib.load(build_if_missing=False), F_._stream()
    assert lib.ggpm_linear_wgrads_batch(0, None, None, 0, None, s) == 0
    assert lib.ggpm_linear_wgrads_batch(-1, None, None, 0, None, s) == C.ERR_ARG
    assert lib.ggpm_linear_wgrads_batch(1, None, None, 0, None, s) == C.ERR_ARG
    rs = np.random.RandomState(3)
    shapes = [(2100, 33, 65, True), (70, 31, 40, False), (6200, 160, 160, True), (2048, 64, 64, True)]      # (M, N, K, db)
    needs = [int(lib.ggpm_gemm_workspace_bytes(N, K, M)) for M, N, K, _ in shapes]
    assert needs[0] > 0 and needs[2] > needs[0] and needs[1] == 0
    data = []
    for M, N, K, db in shapes:
        dpre = _poisoned(rs.standard_normal((M, N)).astype(np.float32), N + 4 - N % 4 if N % 4 else N + 4, 0)[1]
        x = _poisoned(rs.standard_normal((M, K)).astype(np.float32), K + 4 - K % 4 if K % 4 else K + 4, 0)[1]
        data.append((dpre, x))
    for ws_bytes in (None, needs[0], max(needs)):
        ws, words = _workspace(ws_bytes)
        csws = torch.empty(256 * 160, device=_dev())
        items = (F_.WgradItem * len(shapes))()
        outs = []
        for i, ((M, N, K, db), (dpre, x)) in enumerate(zip(shapes, data)):
            dW, dbv = _c_buffer(N, K + 3), torch.full((N + 4,), SENTINEL, device=_dev())
            outs.append((dW, dbv))
            items[i] = F_.WgradItem(dpre.data_ptr(), dpre.stride(0), x.data_ptr(), x.stride(0), dW[1].data_ptr(), K + 3,
                                    dbv.data_ptr() if db else None, M, N, K)
        assert lib.ggpm_linear_wgrads_batch(len(shapes), items, F_._p(ws), ws_bytes or 0, csws.data_ptr(), s) == 0
        torch.cuda.synchronize()
        if ws is not None:
            assert bool((ws[words:] == WS_GUARD).all())
        for (M, N, K, db), (dpre, x), (dW, dbv), need in zip(shapes, data, outs, needs):
            split = ws is not None and need and need <= ws_bytes
            eW, eb = _c_buffer(N, K + 3), torch.full((N + 4,), SENTINEL, device=_dev())
            assert lib.ggpm_gemm(1, 0, N, K, M, dpre.data_ptr(), dpre.stride(0), x.data_ptr(), x.stride(0), eW[1].data_ptr(), K + 3,
                                 K, None, 0, 0, 0, F_._p(ws) if split else None, ws_bytes if split else 0, s) == 0
            if db:
                assert lib.ggpm_colsum(dpre.data_ptr(), dpre.stride(0), M, N, eb.data_ptr(), csws.data_ptr(), s) == 0
            torch.cuda.synchronize()
            assert torch.equal(dW[0].view(torch.int32), eW[0].view(torch.int32)), (M, N, K, ws_bytes)
            assert torch.equal(dbv.view(torch.int32), eb.view(torch.int32)), (M, N, K, ws_bytes)
            want = dpre[:, :N].double().t() @ x[:, :K].double()
            assert float((dW[1][:, :K].double() - want).abs().max() / want.abs().max()) < (2e-6 if M <= 5000 else 5e-6)
