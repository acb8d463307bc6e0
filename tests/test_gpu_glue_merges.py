"""GPU: the merged launches between the encoder's depth loops give the bits of the launches they replace.

Every case compares BITWISE against the composition of the plain entry points the encoder driver used to issue:
  * ggpm_segment_sum_masked      against  copy of the addend + ggpm_segment_sum(accumulate) + ggpm_act_backward
  * ggpm_gemm_grouped_masked     against  copy of the addend + ggpm_gemm_grouped(accumulate) + ggpm_act_backward
  * ggpm_gemm_grouped on operands that do not allow 16-byte loads (one grouped launch of the scalar-load tile)
                                 against  one ggpm_gemm per member
  * ggpm_gemm_ksegments on such operands (one launch that rounds where the chain of launches rounded)
                                 against  that chain of ggpm_gemm calls
  * ggpm_padded_to_csr_pair      against  two ggpm_padded_to_csr
Shapes: M = 1, 17, 33 (ragged, past one 32-row tile), N = 40 (Hp = 48) and 300, CSR rows with 0, 1 and 5 entries."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RELU, TANH = 1, 2


def _dev():
    return torch.device("cuda:0")


def _lib():
    from ggpm_amd import _lib as L
    return L, L.load()


def _F():
    from ggpm_amd import functional as F_
    return F_


def _rand(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(_dev())


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


class GemmEpilogue(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_gemm_epilogue"""
    _fields_ = [("addend", ctypes.c_void_p), ("ld_addend", ctypes.c_int), ("mask_y", ctypes.c_void_p),
                ("mask_out", ctypes.c_void_p), ("ld_mask", ctypes.c_int), ("mask_act", ctypes.c_int),
                ("mask_zero_row0", ctypes.c_int)]


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


def _csr(rs, rows, n_src):
    """rows with 0, 1 and 5 entries in turn (row 0 has none, like the pad row of the encoder's lists); repeats allowed"""
    counts = [(0, 1, 5)[r % 3] for r in range(rows)]
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    col = rs.randint(0, n_src, size=max(int(rowptr[-1]), 1)).astype(np.int32)
    return torch.from_numpy(rowptr).to(_dev()), torch.from_numpy(col).to(_dev())


# ---------------------------------------------------------------------------------------------------- segment sum
@pytest.mark.parametrize("zero_row0", [0, 1])
@pytest.mark.parametrize("act", [RELU, TANH])
@pytest.mark.parametrize("N", [40, 300])
@pytest.mark.parametrize("M", [1, 17, 33])
def test_segment_sum_masked_matches_sum_then_mask(M, N, act, zero_row0):
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(100 * M + N + act)
    Hp, n_src = F_.padded_hidden(N), 29
    src = _rand(rs, n_src, Hp)
    addend = _rand(rs, M, Hp)                      # negative values where the mask is open: about half of them
    y = torch.tanh(_rand(rs, M, Hp)) if act == TANH else torch.relu(_rand(rs, M, Hp))
    rowptr, col = _csr(rs, M, n_src)
    s = F_._stream()
    # reference: copy, accumulate in place, mask
    ref = addend.clone()
    L.check(lib.ggpm_segment_sum(src.data_ptr(), Hp, rowptr.data_ptr(), col.data_ptr(), M, N, ref.data_ptr(), Hp, 1, 0, s), "ss")
    ref_dpre = torch.full((M, Hp), 7.0, device=_dev())
    L.check(lib.ggpm_act_backward(ref.data_ptr(), y.data_ptr(), M, N, Hp, act, zero_row0, ref_dpre.data_ptr(), s), "ab")
    assert bool(((addend[:, :N] < 0) & (y[:, :N] != 0)).any()) or M == 1
    for keep_out in (True, False):
        out = torch.full((M, Hp), 5.0, device=_dev()) if keep_out else None
        dpre = torch.full((M, Hp), 7.0, device=_dev())
        L.check(lib.ggpm_segment_sum_masked(1, _ptrs([src]), Hp, rowptr.data_ptr(), col.data_ptr(), M, N, _ptrs([addend]), Hp,
                                            _ptrs([out]), Hp, 0, _ptrs([y]), _ptrs([dpre]), Hp, act, zero_row0, s), "ssm")
        _same(dpre, ref_dpre, "masked sum")
        if keep_out:
            _same(out[:, :N], ref[:, :N], "plain sum")
            assert bool((out[:, N:] == 5.0).all())           # zero_to = 0: pad columns left alone
    # in place on the accumulated-onto matrix (addend == out), as the motif level's d(hnode) is finished
    out = addend.clone()
    dpre = torch.full((M, Hp), 7.0, device=_dev())
    L.check(lib.ggpm_segment_sum_masked(1, _ptrs([src]), Hp, rowptr.data_ptr(), col.data_ptr(), M, N, _ptrs([out]), Hp,
                                        _ptrs([out]), Hp, 0, _ptrs([y]), _ptrs([dpre]), Hp, act, zero_row0, s), "ssm")
    _same(out, ref, "in-place sum")
    _same(dpre, ref_dpre, "in-place masked sum")


@pytest.mark.parametrize("N,ld_src", [(40, 48), (300, 304), (300, 321)])      # 321: the scalar (unaligned) form
def test_segment_sum_pair_matches_two_sums(N, ld_src):
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(N + ld_src)
    M, Hp, n_src = 33, F_.padded_hidden(N), 11
    srcs = [_rand(rs, n_src, ld_src) for _ in range(2)]
    rowptr, col = _csr(rs, M, n_src)
    s = F_._stream()
    refs = [torch.full((M, Hp), 3.0, device=_dev()) for _ in range(2)]
    for a, o in zip(srcs, refs):
        L.check(lib.ggpm_segment_sum(a.data_ptr(), ld_src, rowptr.data_ptr(), col.data_ptr(), M, N, o.data_ptr(), Hp, 0, Hp, s), "ss")
    outs = [torch.full((M, Hp), 3.0, device=_dev()) for _ in range(2)]
    L.check(lib.ggpm_segment_sum_masked(2, _ptrs(srcs), ld_src, rowptr.data_ptr(), col.data_ptr(), M, N, None, 0, _ptrs(outs), Hp,
                                        Hp, None, None, 0, 0, 0, s), "ssm")
    for o, r in zip(outs, refs):
        _same(o, r, "pair of sums")


# ---------------------------------------------------------------------------------------------------- GEMM epilogue
@pytest.mark.parametrize("zero_row0", [0, 1])
@pytest.mark.parametrize("act", [RELU, TANH])
@pytest.mark.parametrize("N", [40, 300])
@pytest.mark.parametrize("M", [1, 17, 33])
def test_gemm_masked_epilogue_matches_product_then_mask(M, N, act, zero_row0):
    """the pair of input-gradient products of a two-segment Linear, the second finished with addend + mask"""
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(7 * M + N + act)
    Hp, K = F_.padded_hidden(N), N
    dpre_in = _rand(rs, M, Hp)
    W = _rand(rs, K, 2 * N)                        # [K, N + N]: problem i reads columns [i N, (i + 1) N)
    addend = _rand(rs, M, Hp)
    y = torch.tanh(_rand(rs, M, Hp)) if act == TANH else torch.relu(_rand(rs, M, Hp))
    s = F_._stream()

    def problems(c1, c2, acc2):
        arr = (F_.GemmProblem * 2)()
        arr[0] = F_.GemmProblem(dpre_in.data_ptr(), Hp, W.data_ptr(), 2 * N, c1.data_ptr(), Hp, Hp, None, 0, 0, 0)
        arr[1] = F_.GemmProblem(dpre_in.data_ptr(), Hp, W.data_ptr() + 4 * N, 2 * N, c2.data_ptr(), Hp, Hp, None, acc2, 0, 0)
        return arr

    r1, r2 = torch.full((M, Hp), 9.0, device=_dev()), addend.clone()
    L.check(lib.ggpm_gemm_grouped(0, 0, M, N, K, 2, problems(r1, r2, 1), s), "gg")
    ref_dpre = torch.full((M, Hp), 7.0, device=_dev())
    L.check(lib.ggpm_act_backward(r2.data_ptr(), y.data_ptr(), M, N, Hp, act, zero_row0, ref_dpre.data_ptr(), s), "ab")

    c1, c2 = torch.full((M, Hp), 9.0, device=_dev()), torch.full((M, Hp), 9.0, device=_dev())
    dpre = torch.full((M, Hp), 7.0, device=_dev())
    ep = (GemmEpilogue * 2)()
    ep[1] = GemmEpilogue(addend.data_ptr(), Hp, y.data_ptr(), dpre.data_ptr(), Hp, act, zero_row0)
    L.check(lib.ggpm_gemm_grouped_masked(0, 0, M, N, K, 2, problems(c1, c2, 1), ep, s), "ggm")
    _same(c1, r1, "first product")
    _same(c2[:, :N], r2[:, :N], "second product + addend")
    assert bool((c2[:, N:] == 0).all())            # n_pad = Hp: pad columns zeroed, as in the plain call
    _same(dpre, ref_dpre, "masked second output")

    # without an addend (no gradient arrived for that output): the product alone, masked
    r2 = torch.full((M, Hp), 9.0, device=_dev())
    L.check(lib.ggpm_gemm_grouped(0, 0, M, N, K, 2, problems(r1, r2, 0), s), "gg")
    L.check(lib.ggpm_act_backward(r2.data_ptr(), y.data_ptr(), M, N, Hp, act, zero_row0, ref_dpre.data_ptr(), s), "ab")
    ep[1] = GemmEpilogue(None, 0, y.data_ptr(), dpre.data_ptr(), Hp, act, zero_row0)
    L.check(lib.ggpm_gemm_grouped_masked(0, 0, M, N, K, 2, problems(c1, c2, 0), ep, s), "ggm")
    _same(c2, r2, "second product")
    _same(dpre, ref_dpre, "masked second output, no addend")


def test_gemm_masked_refuses_unaligned_operands():
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(3)
    A, W, C = _rand(rs, 17, 48), _rand(rs, 40, 62 + 40), torch.zeros(17, 48, device=_dev())
    arr = (F_.GemmProblem * 1)(F_.GemmProblem(A.data_ptr(), 48, W.data_ptr() + 4 * 62, 102, C.data_ptr(), 48, 48, None, 0, 0, 0))
    ep = (GemmEpilogue * 1)()
    assert lib.ggpm_gemm_grouped_masked(0, 0, 17, 40, 40, 1, arr, ep, F_._stream()) == 3      # GGPM_ERR_UNSUPPORTED
    assert bool((C == 0).all())


# ---------------------------------------------------------------------------------------------------- grouped scalar-load GEMM
@pytest.mark.parametrize("K,H,ld_x", [(62, 300, 64), (38, 40, 40)])
def test_grouped_unaligned_projections_match_single_launches(K, H, ld_x):
    """the atom level's three gate-input projections: W rows of K + H floats (362 / 78: no 16-byte loads), bias on two.
    (The entry point has no way to report WHICH kernel it chose: with these operands ggpm_gemm_grouped takes its one-launch
    gemm_kernel_group branch, which profiles/glue_launch_merges.txt shows running; were it not taken, the per-member launches
    would run and this test would pass for the wrong reason.)"""
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(K + H)
    M, Hp = 33, F_.padded_hidden(H)
    x = _rand(rs, M, ld_x)
    Ws = [_rand(rs, H, K + H), _rand(rs, H, K), _rand(rs, H, K + H)]
    bs = [_rand(rs, H), None, _rand(rs, H)]
    s = F_._stream()
    refs = [torch.full((M, Hp), 2.0, device=_dev()) for _ in range(3)]
    for W, b, o in zip(Ws, bs, refs):
        F_.gemm(0, 1, M, H, K, x, ld_x, W, W.stride(0), o, Hp, Hp, bias=b)
    outs = [torch.full((M, Hp), 2.0, device=_dev()) for _ in range(3)]
    arr = (F_.GemmProblem * 3)()
    for i, (W, b, o) in enumerate(zip(Ws, bs, outs)):
        arr[i] = F_.GemmProblem(x.data_ptr(), ld_x, W.data_ptr(), W.stride(0), o.data_ptr(), Hp, Hp,
                                None if b is None else b.data_ptr(), 0, 0, 0)
    L.check(lib.ggpm_gemm_grouped(0, 1, M, H, K, 3, arr, s), "gg")
    for o, r in zip(outs, refs):
        _same(o, r, "grouped projection")


# ---------------------------------------------------------------------------------------------------- paired CSR build
def test_padded_to_csr_pair_matches_two_calls():
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(11)
    shapes = [(1030, 4), (517, 6)]                 # more rows than the workgroup has threads / fewer
    pads = []
    for rows, width in shapes:
        p = rs.randint(0, rows, size=(rows, width)) * (rs.rand(rows, width) < 0.6)
        p[0] = 0
        pads.append(torch.from_numpy(p.astype(np.int64)).to(_dev()))
    s = F_._stream()

    def bufs():
        return [(torch.full((r + 1,), -1, dtype=torch.int32, device=_dev()),
                 torch.full((r * w,), -1, dtype=torch.int32, device=_dev())) for r, w in shapes]

    ref, got = bufs(), bufs()
    for p, (r, w), (rp, cl) in zip(pads, shapes, ref):
        L.check(lib.ggpm_padded_to_csr(p.data_ptr(), r, w, rp.data_ptr(), cl.data_ptr(), s), "csr")
    (r0, w0), (r1, w1) = shapes
    L.check(lib.ggpm_padded_to_csr_pair(pads[0].data_ptr(), r0, w0, got[0][0].data_ptr(), got[0][1].data_ptr(),
                                        pads[1].data_ptr(), r1, w1, got[1][0].data_ptr(), got[1][1].data_ptr(), s), "pair")
    for (a, b), (c, d) in zip(ref, got):
        assert torch.equal(a, c) and torch.equal(b, d)


# ---------------------------------------------------------------------------------------------------- one-launch read-out
@pytest.mark.parametrize("K1,H,ld1", [(38, 40, 40), (62, 300, 64), (38, 300, 40)])
@pytest.mark.parametrize("M", [17, 33, 130])
def test_unaligned_ksegments_match_the_chain_of_launches(K1, H, ld1, M):
    """the atom read-out relu(x1 W[:, :K1]^T + x2 W[:, K1:]^T + b): W rows of K1 + H floats (78 / 362 / 338), the second block
    at an unaligned column.  The chain: first product + bias stored, second product accumulated onto it, ReLU, row 0 zeroed.
    (As above: that the one-launch branch of ggpm_gemm_ksegments is the one running is shown by the committed trace, not here.)"""
    L, lib = _lib()
    F_ = _F()
    rs = np.random.RandomState(K1 + H + M)
    Hp = F_.padded_hidden(H)
    x1, x2 = _rand(rs, M, ld1), _rand(rs, M, Hp)
    W, b = _rand(rs, H, K1 + H), _rand(rs, H)
    ref = torch.full((M, Hp), 4.0, device=_dev())
    F_.gemm(0, 1, M, H, K1, x1, ld1, W, K1 + H, ref, Hp, Hp, bias=b)
    F_.gemm(0, 1, M, H, H, x2, Hp, W[:, K1:], K1 + H, ref, Hp, H, accumulate=True, act=RELU, zero_row0=True)
    out = torch.full((M, Hp), 4.0, device=_dev())
    F_.gemm_ksegments(1, M, H, [x1, x2], [ld1, Hp], [W, W[:, K1:]], [K1 + H, K1 + H], [K1, H], out, Hp, Hp, bias=b, act=RELU,
                      zero_row0=True)
    _same(out, ref, "two-segment read-out")
    assert bool((out[1:, :H] > 0).any()) and bool((out[0] == 0).all())
