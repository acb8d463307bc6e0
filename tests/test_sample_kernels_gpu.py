"""GPU: the three draw kernels of csrc/sample.hip called on their own through ``_lib``, against the numpy restatement of the
stream (tests/sample_oracle.py) on the seeded cases of tests/sample_kernel_inputs.py -- the cases whose margins and
statistics tests/test_sample_oracle_cpu.py establishes on the CPU.  Topology draws must equal the restatement exactly.
A drawn order must equal the fp64 one on every row whose keys keep the project's decision margin (1e-4), and is a
permutation on all.  Normals are compared under 4 times the distance of numpy's own fp32 evaluation from fp64.  Output
buffers are longer than what a kernel may write and pre-filled with a sentinel."""
import numpy as np
import pytest
import torch

import sample_kernel_inputs as KI
import sample_oracle as SO
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
SENT, ISENT = -777.25, -123456789
ERR_ARG = 1                         # GGPM_ERR_ARG (include/ggpm_hip.h)
P = F_._p
LO, HI = SO.split(KI.SEED)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_ids(ids):
    return dev((np.asarray(ids, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))


def topo(p, bidx, ids, step, seed=KI.SEED):
    n = len(p)
    lo, hi = SO.split(seed)
    out = torch.full((n + 8,), SENT, device=DEV)
    keep = (dev(p), dev(bidx), dev_ids(ids))
    code = _lib.load().ggpm_sample_topo(P(keep[0]), P(keep[1]), P(keep[2]), n, step, lo, hi, P(out), F_._stream())
    assert code == 0
    out = out.cpu().numpy()
    assert (out[n:] == SENT).all()
    return out[:n]


@pytest.mark.parametrize("n", KI.TOPO_N)
def test_topology_draws_equal_the_restatement(n):
    for step in KI.TOPO_STEPS:
        p, bidx, ids = KI.topo_case(n, step)
        got = topo(p, bidx, ids, step)
        assert np.array_equal(got, SO.topo_draws(KI.SEED, ids[bidx], step, p)), (n, step)
        assert not got[p == 0].any() and got[p == 1].all()


def test_topology_draw_frequencies():
    p, bidx, ids = KI.topo_freq_case()
    got = topo(p, bidx, ids, 5)
    assert np.array_equal(got, SO.topo_draws(KI.SEED, ids[bidx], 5, p))
    for row, q in zip(got.reshape(len(KI.FREQ_P), KI.FREQ_N), KI.FREQ_P):
        print("p = %.1f: drew %.5f" % (q, row.mean()))
        assert KI.within_5_sigma(row.sum(), KI.FREQ_N, q)


def beam_order(s, bidx, ids, step):
    """the order kernel on ``hier_topk``'s layout [M, 3k]: the scores' bits, then 2k ints it must not read as scores"""
    M, k = s.shape
    topk = np.full((M, 3 * k), ISENT, np.int32)
    topk[:, :k] = np.ascontiguousarray(s, np.float32).view(np.int32)
    out = torch.full((M * k + 8,), ISENT, dtype=torch.int32, device=DEV)
    keep = (dev(topk), dev(bidx), dev_ids(ids))
    code = _lib.load().ggpm_sample_beam_order(P(keep[0]), P(keep[1]), P(keep[2]), M, k, step, LO, HI, P(out),
                                              F_._stream())
    assert code == 0
    out = out.cpu().numpy()
    assert (out[M * k:] == ISENT).all()
    return out[:M * k].reshape(M, k).astype(np.int64)


@pytest.mark.parametrize("M", KI.ORDER_M)
@pytest.mark.parametrize("k", KI.ORDER_K)
def test_beam_orders_equal_the_restatement(M, k):
    (s, bidx, ids, step), want, keep = KI.order_expected(M, k)
    got = beam_order(s, bidx, ids, step)
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(k), (M, 1)))      # every row a permutation
    assert (~keep).sum() <= KI.SKIP_CAP * M
    assert np.array_equal(got[keep], want[keep])
    masked = s < -500
    for r in range(M):
        n = int(masked[r].sum())
        assert n == 0 or set(got[r, k - n:]) == set(np.nonzero(masked[r])[0])      # masked entries come last


def test_the_host_sampler_ranks_masked_tails_as_the_kernel_does():
    """rows with two and more masked entries: the ``sampler=`` seam's restated sampler, fed as the decode loop feeds it,
    gives the kernel's order, tail included"""
    (s, bidx, ids, step), _, keep = KI.order_expected(65, 16)
    sampler = SO.Sampler(KI.SEED)
    s64 = s.astype(np.float64)
    want = sampler.order(step, [int(v) for v in ids[bidx]], np.exp(s64), s64)
    assert sampler.n_masked_rows >= 16
    assert np.array_equal(beam_order(s, bidx, ids, step)[keep], want[keep])


def test_equal_scores_with_equal_words_go_to_the_lower_index():
    s, bidx, ids, step = KI.tie_case()
    got = beam_order(s, bidx, ids, step)
    assert np.array_equal(got, SO.beam_order(KI.SEED, ids[bidx], step, s)[0])
    pos = list(got[0])
    assert pos.index(KI.TIE_SLOTS[1]) == pos.index(KI.TIE_SLOTS[0]) + 1


def test_beam_order_frequencies():
    s, bidx, ids, step = KI.freq_case()
    first, second = KI.check_frequencies(beam_order(s, bidx, ids, step))
    print("first places", first, "second places after entry 0", second)


def normal(rows, cols, ids, seed, ld=None):
    ld = cols + 3 if ld is None else ld
    lo, hi = SO.split(seed)
    out = torch.full((rows + 1, ld), SENT, device=DEV)
    keep = dev_ids(ids)
    code = _lib.load().ggpm_sample_normal(P(out), rows, cols, ld, P(keep), lo, hi, F_._stream())
    assert code == 0
    out = out.cpu().numpy()
    assert (out[:rows, cols:] == SENT).all() and (out[rows] == SENT).all()      # the padding and the next row
    return out[:rows, :cols]


@pytest.mark.parametrize("rows,cols", KI.NORMAL_SHAPES)
def test_normals_equal_the_restatement(rows, cols):
    ids, want, bound = KI.normal_expected(rows, cols)
    got = normal(rows, cols, ids, KI.normal_seed(rows, cols))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%d x %d: distance %.3e, bound %.3e" % (rows, cols, err, bound))
    assert err <= bound


def test_normals_moments_and_row_invariance():
    z = normal(4096, 64, np.arange(4096), KI.SEED, ld=64)
    print("mean %.5f variance %.5f" % KI.check_moments(z))
    ids = KI.normal_ids()
    perm = np.random.RandomState(1).permutation(len(ids))
    a, b = normal(len(ids), 24, ids, KI.SEED), normal(len(ids), 24, ids[perm], KI.SEED)
    assert np.array_equal(b, a[perm])       # a row's values follow its id, not its position
    assert np.array_equal(normal(3, 24, ids[[200, 7, 31]], KI.SEED), a[[200, 7, 31]])       # ... nor the number of rows
    assert np.array_equal(F_.sample_normal(5, 24, LO, HI, ids=ids[:5], device=DEV).cpu().numpy(), a[:5])


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    f = torch.full((64,), SENT, device=DEV)
    i = torch.full((64,), ISENT, dtype=torch.int32, device=DEV)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = torch.full((16,), 0.5, device=DEV)
    s = F_._stream()
    assert lib.ggpm_sample_topo(P(p), P(z), P(z), 0, 0, LO, HI, P(f), s) == ERR_ARG                 # n = 0
    assert lib.ggpm_sample_topo(P(p), P(z), None, 4, 0, LO, HI, P(f), s) == ERR_ARG                 # a null pointer
    assert lib.ggpm_sample_topo(P(p), P(z), P(z), 4, 0, LO, HI, None, s) == ERR_ARG
    topk = torch.zeros(3 * 17, dtype=torch.int32, device=DEV)
    assert lib.ggpm_sample_beam_order(P(topk), P(z), P(z), 1, 17, 0, LO, HI, P(i), s) == ERR_ARG    # k = 17
    assert lib.ggpm_sample_beam_order(P(topk), P(z), P(z), 1, 0, 0, LO, HI, P(i), s) == ERR_ARG     # k = 0
    assert lib.ggpm_sample_beam_order(P(topk), P(z), P(z), 0, 5, 0, LO, HI, P(i), s) == ERR_ARG     # M = 0
    assert lib.ggpm_sample_beam_order(None, P(z), P(z), 1, 5, 0, LO, HI, P(i), s) == ERR_ARG
    assert lib.ggpm_sample_normal(P(f), 0, 4, 4, P(z), LO, HI, s) == ERR_ARG                        # rows = 0
    assert lib.ggpm_sample_normal(P(f), 2, 8, 4, P(z), LO, HI, s) == ERR_ARG                        # ld < cols
    assert lib.ggpm_sample_normal(P(f), 2, 4, 4, None, LO, HI, s) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all() and (i.cpu().numpy() == ISENT).all()                     # nothing ran
