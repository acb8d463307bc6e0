"""CPU: the numerics of the closed-form hidden-half weight gradients of a tree-side level at its fixed point.

In the fixed-slot regime (ggpm_level_opts.fixed_slot) dW = (sum_t D_t)^T X* replaces the stacked contraction
sum_t D_t^T X* (K = C E rows).  The slot sum is kept as an unevaluated fp32 pair hi + lo (two-sum per term,
mpn_gru.hip: sum_slots_pair_k) and contracted as [hi; lo]^T [X*; X*] by gemm_small_v3 (K = 2 E, one accumulator chain per
wave: the four waves of a workgroup take the four quarters of every 64-wide k-step, partial tiles summed pairwise).  Both
steps are restated here in numpy fp32, on operands shaped like the backward's (E = 600 messages, H = 300, C = 9 slots whose
magnitudes fall by step and whose rows go exactly zero once a message's chain is exhausted).  The bound the GPU tests hold
these tensors to is 2e-6 x max|.|.  Two things are pinned, each measured the way the change request measured it:

* the form the library runs, against fp64: at least 4x inside the bound;
* a plain fp32 pre-sum followed by the same product, against an 8-way blocked stacked fp32 contraction (the un-hinted
  run's shape: K = C E in eight blocks, each one sequential fp32 chain) -- what the GPU tests compare, hinted against
  un-hinted, both fp32: NOT 4x inside the bound.  That reading is why the slot sum was not allowed to round on its own.

Measured here (max |difference| / max |dW|, seeds 0-2; bound / 4 = 5e-7):
    hi + lo pair against fp64                          2.9e-7  3.4e-7  3.2e-7
    plain pre-sum against the blocked stacked fp32     8.2e-7  8.4e-7  9.7e-7
    for the record: the blocked stacked contraction against fp64 8.5e-7  8.4e-7  8.8e-7; the plain pre-sum against fp64
    2.9e-7  3.4e-7  3.2e-7; the slot sum's own share (product in fp64) pair 1.6e-15 - 2.3e-15, plain 2.9e-8 - 3.0e-8.
So the second figure is mostly the accumulation error of the K = C E reference chain, which a comparison of two fp32 runs
always carries; the pair form takes the slot sum itself out of the budget (2e-15 against 3e-8) at the price of one more K
segment in a 20 us second-stream launch."""
import numpy as np

E, H, C = 600, 300, 9
BOUND = 2e-6
MARGIN = 4.0


def _operands(seed, decay=0.5):
    rs = np.random.RandomState(seed)
    live_steps = rs.randint(1, C + 1, size=E)          # row r is nonzero in the first live_steps[r] backward steps
    D = np.zeros((C, E, H), np.float32)
    for k in range(C):
        live = live_steps > k
        D[k, live] = (rs.standard_normal((int(live.sum()), H)) * decay ** k).astype(np.float32)
    X = np.tanh(rs.standard_normal((E, H))).astype(np.float32)
    return D, X


def _gemm_tn_small_v3(A, B):
    """A^T B in fp32 the way gemm_small_v3 accumulates it: wave w owns k with (k % 64) // 16 == w, sequentially"""
    acc = [np.zeros((A.shape[1], B.shape[1]), np.float32) for _ in range(4)]
    for k in range(A.shape[0]):
        acc[(k % 64) // 16] += np.outer(A[k], B[k])
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _slot_sums(D):
    """-> (plain fp32 sum, hi, lo), slots in the kernel's order (the first slot read is the last backward step's)"""
    plain = D[0].copy()
    hi, lo = D[0].copy(), np.zeros_like(D[0])
    for t in range(1, D.shape[0]):
        plain = plain + D[t]
        hi, e = _two_sum(hi, D[t])
        lo = lo + e
    return plain, hi, lo


def _errors(seed):
    D, X = _operands(seed)
    D = D[::-1].copy()                                  # stash slot lo - 1 holds the LAST backward step (smallest magnitudes)
    ref = np.einsum("tek,eh->kh", D.astype(np.float64), X.astype(np.float64))
    scale = np.abs(ref).max()
    plain, hi, lo = _slot_sums(D)
    X64 = X.astype(np.float64)
    return {
        "pair": np.abs(_gemm_tn_small_v3(np.concatenate([hi, lo]), np.concatenate([X, X])) - ref).max() / scale,
        "plain": np.abs(_gemm_tn_small_v3(plain, X) - ref).max() / scale,
        "pair_sum_only": np.abs((hi.astype(np.float64) + lo.astype(np.float64)).T @ X64 - ref).max() / scale,
        "plain_sum_only": np.abs(plain.astype(np.float64).T @ X64 - ref).max() / scale,
    }


def test_two_sum_pair_is_exact_per_term():
    rs = np.random.RandomState(0)
    a = (rs.standard_normal(4096) * 10.0 ** rs.randint(-6, 6, 4096)).astype(np.float32)
    b = (rs.standard_normal(4096) * 10.0 ** rs.randint(-6, 6, 4096)).astype(np.float32)
    s, e = _two_sum(a, b)
    assert s.dtype == np.float32 and e.dtype == np.float32
    assert np.array_equal(s.astype(np.float64) + e.astype(np.float64), a.astype(np.float64) + b.astype(np.float64))


def test_pair_presum_keeps_the_margin():
    for seed in range(3):
        err = _errors(seed)
        print("seed %d: %s" % (seed, ", ".join("%s %.3e" % kv for kv in sorted(err.items()))))
        assert err["pair"] <= BOUND / MARGIN, (seed, err)
        assert err["pair_sum_only"] <= 1e-12, (seed, err)          # the slot sum itself does not round


def _stacked_blocked_fp32(D, X, ways=8):
    """sum_t D_t^T X as ONE fp32 contraction over the C E stacked rows, in `ways` blocks of one sequential chain each"""
    A = D.reshape(-1, D.shape[2])
    out = np.zeros((A.shape[1], X.shape[1]), np.float32)
    for blk in np.array_split(np.arange(A.shape[0]), ways):
        acc = np.zeros_like(out)
        for k in blk:
            acc += np.outer(A[k], X[k % X.shape[0]])
        out = out + acc
    return out


def test_plain_presum_lacks_the_margin():
    """A plain fp32 pre-sum of the nine slots followed by the product, against the 8-way blocked stacked contraction."""
    for seed in range(3):
        D, X = _operands(seed)
        D = D[::-1].copy()
        scale = np.abs(np.einsum("tek,eh->kh", D.astype(np.float64), X.astype(np.float64))).max()
        plain, _, _ = _slot_sums(D)
        diff = np.abs(_gemm_tn_small_v3(plain, X) - _stacked_blocked_fp32(D, X)).max() / scale
        print("seed %d: plain pre-sum against the blocked stacked contraction %.3e, bound / 4 = %.1e" % (seed, diff, BOUND / MARGIN))
        assert diff > BOUND / MARGIN, (seed, diff)
