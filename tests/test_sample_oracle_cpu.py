"""CPU: the numpy restatement of the seeded stream (tests/sample_oracle.py) on its own -- the integer mixing against plain
Python integers, the statistical checks the GPU tests make on the kernels' output passing on the restatement alone, and
every seeded case of tests/sample_kernel_inputs.py keeping the margins the GPU tests rely on."""
import numpy as np
import pytest

import sample_kernel_inputs as KI
import sample_oracle as SO


def _fmix(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ h >> 16


def _word(seed, site, i, step, slot):
    """the DESIGN text in Python integers"""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    base = _fmix(_fmix((i * 0x9E3779B1 + lo) & 0xFFFFFFFF) ^ ((hi + site * 0x7F4A7C15) & 0xFFFFFFFF))
    return _fmix((base + (step * 64 + slot) * 0x9E3779B1) & 0xFFFFFFFF) >> 8


def test_words_are_the_design_text_in_integers():
    rs = np.random.RandomState(0)
    ids = [0, 1, 0xFFFFFFFF, 0x80000000] + [int(v) for v in rs.randint(0, 1 << 31, 20)]
    for site in (SO.SITE_TOPO, SO.SITE_BEAM, SO.SITE_PRIOR):
        for step in (0, 1, 149, 1 << 27):
            got = SO.words(KI.SEED, site, np.asarray(ids).reshape(-1, 1), step, np.arange(16).reshape(1, 16))
            want = [[_word(KI.SEED, site, i, step, q) for q in range(16)] for i in ids]
            assert np.array_equal(got, np.asarray(want, np.uint64))
    assert SO.words(KI.SEED, SO.SITE_TOPO, ids, 0, 0).max() < 1 << 24
    # the three sites, two seeds that differ in one half only, two steps and two slots give different words
    a = SO.words(KI.SEED, SO.SITE_TOPO, np.arange(1000), 0, 0)
    for other in (SO.words(KI.SEED, SO.SITE_BEAM, np.arange(1000), 0, 0), SO.words(KI.SEED ^ 1, SO.SITE_TOPO, np.arange(1000), 0, 0),
                  SO.words(KI.SEED ^ 1 << 32, SO.SITE_TOPO, np.arange(1000), 0, 0), SO.words(KI.SEED, SO.SITE_TOPO, np.arange(1000), 1, 0),
                  SO.words(KI.SEED, SO.SITE_TOPO, np.arange(1000), 0, 1)):
        assert (a == other).mean() < 0.01


def test_topology_draw_edges_and_frequencies():
    for n in KI.TOPO_N:
        for step in KI.TOPO_STEPS:
            p, bidx, ids = KI.topo_case(n, step)
            d = SO.topo_draws(KI.SEED, ids[bidx], step, p)
            u = SO.topo_uniforms(KI.SEED, ids[bidx], step)
            assert not d[p == 0].any() and d[p == 1].all()
            assert not d[p.astype(np.float64) == u].any() and d[p.astype(np.float64) == u + 2.0 ** -24].all()
    p, bidx, ids = KI.topo_case(257, 0)     # (the boundary values survive the rounding to fp32: they are fp32 values)
    assert (p.astype(np.float64) == SO.topo_uniforms(KI.SEED, ids[bidx], 0)).sum() >= 30
    p, bidx, ids = KI.topo_freq_case()
    d = SO.topo_draws(KI.SEED, ids[bidx], 5, p).reshape(len(KI.FREQ_P), KI.FREQ_N)
    for row, q in zip(d, KI.FREQ_P):
        assert KI.within_5_sigma(row.sum(), KI.FREQ_N, q), (q, row.mean())


@pytest.mark.parametrize("M", KI.ORDER_M)
@pytest.mark.parametrize("k", KI.ORDER_K)
def test_order_cases_keep_their_margin_in_fp32(M, k):
    (s, bidx, ids, step), order, keep = KI.order_expected(M, k)
    assert (~keep).sum() <= KI.SKIP_CAP * M
    o32, _ = SO.beam_order(KI.SEED, ids[bidx], step, s, np.float32)
    assert np.array_equal(o32[keep], order[keep])
    assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(k), (M, 1)))
    masked = s < -500
    if k > 2 and M > 1:
        assert masked.any() and (s[:, 0] == s[:, 1]).any()
    for r in range(M):          # masked entries come last
        n = int(masked[r].sum())
        assert n == 0 or set(order[r, k - n:]) == set(np.nonzero(masked[r])[0])


def test_equal_scores_with_equal_words_go_to_the_lower_index():
    s, bidx, ids, step = KI.tie_case()
    a, b = KI.TIE_SLOTS
    m = SO.words(KI.SEED, SO.SITE_BEAM, ids, step, np.arange(16))
    assert a < b and m[a] == m[b] and s[0, a] == s[0, b]
    order, _ = SO.beam_order(KI.SEED, ids[bidx], step, s)
    keys = SO.beam_keys(KI.SEED, ids[bidx], step, s)[0]
    pos = list(order[0])
    assert pos.index(b) == pos.index(a) + 1
    gaps = -np.diff(keys[order[0]])
    assert np.sort(gaps)[0] == 0 and np.sort(gaps)[1] >= SO.MARGIN
    assert np.array_equal(SO.beam_order(KI.SEED, ids[bidx], step, s, np.float32)[0], order)


def test_order_frequencies_are_plackett_luce():
    s, bidx, ids, step = KI.freq_case()
    order, _ = SO.beam_order(KI.SEED, ids[bidx], step, s)
    KI.check_frequencies(order)


def test_normals():
    for rows, cols in KI.NORMAL_SHAPES:
        ids, z64, bound = KI.normal_expected(rows, cols)
        assert z64.shape == (rows, cols) and 1e-7 < bound < 1e-5, (rows, cols, bound)
    # DESIGN.md quotes the bound of the largest case
    assert abs(KI.normal_expected(257, 56)[2] - 4.94e-6) < 1e-8
    ids = KI.normal_ids()
    z = SO.normals(KI.SEED, np.arange(4096), 64)
    KI.check_moments(z)
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0))         # u1 >= 2^-24 bounds the radius
    perm = np.random.RandomState(1).permutation(len(ids))
    assert np.array_equal(SO.normals(KI.SEED, ids[perm], 8), SO.normals(KI.SEED, ids, 8)[perm])
