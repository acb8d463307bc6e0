"""The seeded inputs of the draw-kernel tests (tests/test_sample_kernels_gpu.py), shared with the CPU test that shows the
restatement alone passing every statistical check and every seed keeping its margins (tests/test_sample_oracle_cpu.py).
Every figure a GPU test compares against is computed here, on the CPU, once per session."""
import functools

import numpy as np

import sample_oracle as SO

SEED = 0x0123456789ABCDEF
TOPO_N = (1, 63, 64, 65, 257, 1030)     # one row; around the 64-lane wave; past one 256-thread workgroup; past four
TOPO_STEPS = (0, 1, 149)
ORDER_K = (1, 2, 5, 16)
ORDER_M = (1, 65)
NORMAL_SHAPES = ((1, 1), (3, 7), (65, 24), (257, 56))
FREQ_N = 65536
FREQ_P = (0.1, 0.5, 0.9)
WEIGHTS = (0.5, 0.25, 0.125, 0.0625, 0.0625)
ORDER_SALT = {(65, 16): 1}              # (the unsalted rows of this case have two near-ties: 3 % of 65 rows)
SKIP_CAP = 0.02                         # rows of an order case whose smallest adjacent key gap is below SO.MARGIN
# an id whose beam words of step TIE_STEP agree at two slots (found by tie_search below): equal scores there give equal keys
TIE_ID, TIE_STEP, TIE_SLOTS = 255512, 3, (3, 13)


def sample_ids(rs, n):
    """n distinct, non-contiguous, unsorted sample ids, some above 2^31"""
    ids = rs.choice(1 << 22, size=n, replace=False).astype(np.int64) * 1021 + 17
    ids[::5] += 1 << 31
    return ids & 0xFFFFFFFF


def topo_case(n, step):
    """-> (p [n] fp32, bidx [n], ids [B]): B = n + 9 molecules, the rows a shuffled subset of them; p cycles through 0, 1,
    the row's own uniform m 2^-24 (the draw must be 0: the compare is strict), the next value above it (the draw must
    be 1) and uniform random values"""
    rs = np.random.RandomState(1000 * n + step)
    ids = sample_ids(rs, n + 9)
    bidx = rs.permutation(n + 9)[:n].astype(np.int32)
    u = SO.topo_uniforms(SEED, ids[bidx], step)
    p = rs.uniform(0, 1, n)
    kind = (np.arange(n) + step) % 7
    p = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, np.where(kind == 2, u, np.where(kind == 3, u + 2.0 ** -24, p))))
    return p.astype(np.float32), bidx, ids


def topo_freq_case():
    """FREQ_N ids at each of FREQ_P -> (p [3 FREQ_N] fp32, bidx, ids [FREQ_N])"""
    rs = np.random.RandomState(7)
    ids = sample_ids(rs, FREQ_N)
    bidx = np.tile(np.arange(FREQ_N, dtype=np.int32), len(FREQ_P))
    return np.repeat(np.asarray(FREQ_P, np.float32), FREQ_N), bidx, ids


def within_5_sigma(count, n, p):
    return abs(count - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def order_case(M, k):
    """-> (scores [M, k] fp32, bidx [M], ids [B], step): rows of a log-softmax over 24 classes, its k largest in
    descending order as hier_topk lists them; every fourth row from the second has a masked tail (about -1000), every
    fourth from the third two exactly equal leading scores"""
    rs = np.random.RandomState(100 * M + k + ORDER_SALT.get((M, k), 0))
    ids = sample_ids(rs, M + 5)
    bidx = rs.permutation(M + 5)[:M].astype(np.int32)
    x = 2.0 * rs.standard_normal((M, 24))
    ls = x - x.max(axis=1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(axis=1, keepdims=True))
    s = -np.sort(-ls, axis=1)[:, :k]
    for r in range(M):
        if r % 4 == 1 and k > 2:
            t = (k + 2) // 3
            s[r, k - t:] = -1000.0 + s[r, k - t:]
        if r % 4 == 2 and k > 1:
            s[r, 1] = s[r, 0]
    return s.astype(np.float32), bidx, ids, 3 + k


def order_expected(M, k):
    """-> (the case, order [M, k] of the fp64 restatement, rows to compare: those whose keys keep SO.MARGIN)"""
    s, bidx, ids, step = order_case(M, k)
    order, gaps = SO.beam_order(SEED, ids[bidx], step, s)
    return (s, bidx, ids, step), order, gaps >= SO.MARGIN


def tie_case():
    """one row with two equal scores at TIE_SLOTS keyed by TIE_ID at TIE_STEP, k = 16 -> (scores [1, 16] fp32, bidx, ids, step)"""
    s = np.linspace(-1.0, -4.0, 16)
    s[list(TIE_SLOTS)] = -2.5
    return s.astype(np.float32)[None, :], np.zeros(1, np.int32), np.asarray([TIE_ID], np.int64), TIE_STEP


def tie_search(limit=1 << 20):
    """the first (id, slots) below ``limit`` whose beam words of TIE_STEP collide (python tests/sample_kernel_inputs.py)"""
    for lo in range(0, limit, 1 << 16):
        ids = np.arange(lo, lo + (1 << 16))
        m = SO.words(SEED, SO.SITE_BEAM, ids.reshape(-1, 1), TIE_STEP, np.arange(16).reshape(1, 16))
        srt = np.sort(m, axis=1)
        hit = np.nonzero((np.diff(srt, axis=1) == 0).any(axis=1))[0]
        if len(hit):
            row = m[hit[0]]
            v = [x for x in row if (row == x).sum() > 1][0]
            return int(ids[hit[0]]), tuple(int(q) for q in np.nonzero(row == v)[0])
    return None


def freq_case():
    """FREQ_N rows of log(WEIGHTS) -> (scores [FREQ_N, 5] fp32, bidx, ids, step)"""
    rs = np.random.RandomState(11)
    ids = sample_ids(rs, FREQ_N)
    s = np.tile(np.log(np.asarray(WEIGHTS)), (FREQ_N, 1)).astype(np.float32)
    return s, np.arange(FREQ_N, dtype=np.int32), ids, 2


def check_frequencies(order):
    """first places against WEIGHTS, and second places among the rows that picked entry 0 first against the renormalised
    rest, both within 5 sigma -> the observed frequencies"""
    w = np.asarray(WEIGHTS)
    n = len(order)
    first = np.bincount(order[:, 0], minlength=5)
    for q in range(5):
        assert within_5_sigma(first[q], n, w[q]), ("first place", q, first[q] / n, w[q])
    sub = order[order[:, 0] == 0]
    second = np.bincount(sub[:, 1], minlength=5)
    assert second[0] == 0
    for q in range(1, 5):
        assert within_5_sigma(second[q], len(sub), w[q] / (1.0 - w[0])), ("second place", q, second[q] / len(sub))
    return first / n, second / len(sub)


@functools.lru_cache(maxsize=None)
def normal_ids():
    return sample_ids(np.random.RandomState(5), 257)


def normal_seed(rows, cols):
    """the 1 x 1 case has a seed of its own: one whose single element does not happen to round exactly in numpy's fp32,
    which would leave a libm that differs by an ulp no room under 4 times that distance"""
    return SEED + 32 if (rows, cols) == (1, 1) else SEED


@functools.lru_cache(maxsize=None)
def normal_expected(rows, cols):
    """-> (ids [rows], fp64 normals [rows, cols], bound: 4 times the largest distance of the numpy fp32 evaluation of the
    same elements from fp64)"""
    ids, seed = normal_ids()[:rows], normal_seed(rows, cols)
    z64 = SO.normals(seed, ids, cols)
    z32 = SO.normals(seed, ids, cols, np.float32)
    return ids, z64, 4.0 * float(np.abs(z32.astype(np.float64) - z64).max())


def check_moments(z):
    """mean 0 and variance 1 of N standard normals within 5 sigma (1 / sqrt N and sqrt(2 / N)) -> (mean, variance)"""
    z = np.asarray(z, np.float64).reshape(-1)
    n = z.size
    assert abs(z.mean()) <= 5.0 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), z.var()
    return z.mean(), z.var()


if __name__ == "__main__":
    print("tie:", tie_search())
    for shape in NORMAL_SHAPES:
        print("normal bound", shape, normal_expected(*shape)[2])
