"""GPU: the four entries of csrc/latent_dims.hip called on their own against the fp64 numpy forms of
tests/latent_dims_oracle.py, at the smallest shapes that can break them: one molecule, fewer than a wave, past one wave of
b-strided lanes, several strides; one column, a few, past one wave of j-strided lanes (and past the 16 waves of the free-bits
workgroup); pre_var of both signs and 0; a row that is exactly zero; a column of means near 100 with spread 0.01.

Bounds, with u = 2^-24 (half an fp32 ulp, relative), expf taken as 2u, and fp64(n) = (n + 16) * 2^-52 what the fp64 additions
of n addends plus the shuffle tree, the accumulator additions and the divisions can add, relative to the sum of the
addends' magnitudes:
  * the fp32 addend a = 1 + lv - m^2 - expf(lv) rounds at 1 + lv, at m^2, at the first difference t2, in expf (2u) and at
    the last difference:  err_a = u (|1 + lv| + m^2 + |t2| + 2 e^lv + |a|), err_kd = err_a / 2  (fewer if the compiler fuses).
  * a column mean of kl_dim (kl_dims, klbar):  sum_b |w_b| err_kd / B + fp64(B) sum_b |w_b kd| / B + u |value|.
  * mu_mean: fp64(N) mean|m| + u |value|;  sigma2_mean: 2u mean(e^lv) + fp64(N) mean(e^lv) + u |value|.
  * mu_var = E[m^2] - mu^2 is formed in fp64 from fp32 inputs whose squares are exact: the sums' and the product's fp64
    errors are relative to E[m^2], not to the variance:  4 fp64(N) E[m^2] + u |value|.  For the cancelling column (means
    near 100, spread 0.01, N = 300) that is 4 * 316 * 2^-52 * 1e4 = 2.8e-9 against a variance of 1e-4: 2.8e-5 relative, which
    is asserted to stay under 1e-4 of that column's OWN value, not only norm-wise.
  * agg_var: the two bounds above + u |value|.
  * term = sum_j max(lambda, klbar_j): sum_j (the klbar bound without its final rounding, where the column is not free)
    + fp64(L) sum_j |addend| + u |term|.
  * backward: c = g w_b / B is formed in fp64; dmean = fl(c m): (u + 4 * 2^-52) |ref|; dpre_var = -+ c (1 - expf(lv)) / 2:
    |c| u e^lv + (u + 4 * 2^-52) |ref|.
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure.  The measured maxima are printed beside
the bounds."""
import numpy as np
import pytest
import torch

import latent_dims_oracle as D
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
E64 = 2.0 ** -52
SENT = -777.25
ERR_ARG = 1
P = F_._p
SLACK = 1.0 + 2.0 ** -10
BS, LS = [1, 3, 65, 300], [1, 8, 65]
CANCEL = 3              # the column of means near 100 (L >= 8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def fp64(n):
    return (n + 16) * E64


def zero_cols(L):
    """the columns in which the last molecule (B >= 3) is exactly zero: all but the cancelling one, which keeps its mean"""
    return [j for j in range(L) if not (L >= 8 and j == CANCEL)]


def case(B, L):
    rs = np.random.RandomState(B * 1000 + L)
    mean = rs.standard_normal((B, L)).astype(np.float32)
    pv = (rs.standard_normal((B, L)) * 1.5).astype(np.float32)
    flat = pv.reshape(-1)
    flat[::5] = 0.0                                         # pre_var exactly 0 (both signs elsewhere)
    if L >= 8:
        mean[:, CANCEL] = (100.0 + 0.01 * rs.standard_normal(B)).astype(np.float32)
    if B >= 3:
        mean[B - 1, zero_cols(L)], pv[B - 1, zero_cols(L)] = 0.0, 0.0      # a row whose kl_dim is exactly 0
    w = (rs.rand(B) * 3 + 0.1).astype(np.float32)
    return mean, pv, w


def err_kd(mean, pv):
    m, p = mean.astype(np.float64), pv.astype(np.float64)
    lv = -np.abs(p)
    e = np.exp(lv)
    t1 = 1.0 + lv
    t2 = t1 - m * m
    return 0.5 * U * (np.abs(t1) + m * m + np.abs(t2) + 2 * e + np.abs(t2 - e))


def klbar_bound(mean, pv, w, final=True):
    """[L]: the bound of a weighted column mean of kl_dim (``final``: with the rounding where it is stored)"""
    B = mean.shape[0]
    ww = np.ones(B) if w is None else np.abs(w.astype(np.float64))
    kd = np.abs(D.kl_dim(mean, pv))
    b = (ww[:, None] * err_kd(mean, pv)).sum(axis=0) / B + fp64(B) * (ww[:, None] * kd).sum(axis=0) / B
    return (b + (U * np.abs(D.klbar(mean, pv, w)) if final else 0.0)) * SLACK


def stat_bounds(mean, pv, out64):
    """[5, L]: the bounds of the five rows of ggpm_latent_dim_finish's output for the molecules (mean, pv)"""
    m = mean.astype(np.float64)
    N = m.shape[0]
    e = np.exp(-np.abs(pv.astype(np.float64)))
    b = np.zeros_like(out64)
    b[0] = klbar_bound(mean, pv, None)
    b[1] = fp64(N) * np.abs(m).mean(axis=0) + U * np.abs(out64[1])
    b[2] = 4 * fp64(N) * (m * m).mean(axis=0) + U * np.abs(out64[2])
    b[3] = (2 * U + fp64(N)) * e.mean(axis=0) + U * np.abs(out64[3])
    b[4] = 4 * fp64(N) * (m * m).mean(axis=0) + (2 * U + fp64(N)) * e.mean(axis=0) + U * np.abs(out64[4])
    return b * SLACK


# ---------------------------------------------------------------------------------------------- raw calls, sentinels behind
def accumulate(chunks, L):
    """zeroed acc [5, L] (+ 4 sentinels behind it), one ggpm_latent_dim_accumulate per (mean, pv) chunk -> the whole buffer"""
    lib, s = _lib.load(), F_._stream()
    acc = torch.full((5 * L + 4,), SENT, dtype=torch.float64, device=DEV)
    acc[:5 * L] = 0.0
    for mean, pv in chunks:
        m, p = dev(mean), dev(pv)                                             # (held until the launch is issued)
        assert lib.ggpm_latent_dim_accumulate(P(m), P(p), mean.shape[0], L, P(acc), s) == 0
    return acc


def finish(acc, L, thr):
    lib, s = _lib.load(), F_._stream()
    out = torch.full((5 * L + 3,), SENT, dtype=torch.float32, device=DEV)
    na = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    assert lib.ggpm_latent_dim_finish(P(acc), L, thr, P(out), P(na), s) == 0
    o, n = out.cpu().numpy(), na.cpu().numpy()
    assert (o[5 * L:] == SENT).all() and (n[1:] == -7).all()                 # nothing behind out / n_active is written
    assert (acc[5 * L:].cpu().numpy() == SENT).all()
    return o[:5 * L].reshape(5, L), int(n[0])


def free_bits(mean, pv, w, lam):
    lib, s = _lib.load(), F_._stream()
    B, L = mean.shape
    kd = torch.full((L + 3,), SENT, dtype=torch.float32, device=DEV)
    term = torch.full((3,), SENT, dtype=torch.float32, device=DEV)
    m, p, ww = dev(mean), dev(pv), dev(w) if w is not None else None
    assert lib.ggpm_free_bits_kl(P(m), P(p), P(ww), B, L, lam, P(kd), P(term), s) == 0
    k, t = kd.cpu().numpy(), term.cpu().numpy()
    assert (k[L:] == SENT).all() and (t[1:] == SENT).all()
    return k[:L].copy(), t[:1].copy()


def free_bits_backward(mean, pv, w, lam, g, kl_dims):
    lib, s = _lib.load(), F_._stream()
    B, L = mean.shape
    dm = torch.full((B * L + 5,), SENT, dtype=torch.float32, device=DEV)
    dp = torch.full((B * L + 5,), SENT, dtype=torch.float32, device=DEV)
    m, p, ww = dev(mean), dev(pv), dev(w) if w is not None else None
    gate = dev(kl_dims) if kl_dims is not None else None
    gg = dev(np.array([g], np.float32)) if g is not None else None
    assert lib.ggpm_free_bits_kl_backward(P(m), P(p), P(ww), P(gate), B, L, lam, P(gg), P(dm), P(dp), s) == 0
    a, b = dm.cpu().numpy(), dp.cpu().numpy()
    assert (a[B * L:] == SENT).all() and (b[B * L:] == SENT).all()
    return a[:B * L].reshape(B, L).copy(), b[:B * L].reshape(B, L).copy()


# ---------------------------------------------------------------------------------------------- accumulate + finish
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_statistics_equal_fp64_within_the_derived_bounds(B, L):
    mean, pv, _ = case(B, L)
    if B * L >= 8:
        assert (pv > 0).any() and (pv < 0).any()
    assert (pv == 0).any()
    want, _ = D.finish(D.accumulate(mean, pv), 0.01)
    acc = accumulate([(mean, pv)], L)
    assert (f64(acc[:L]) == B).all()
    got, _ = finish(acc, L, 0.01)
    bound = stat_bounds(mean, pv, want)
    err = np.abs(got.astype(np.float64) - want)
    for r, what in enumerate(("kl_dims", "mu_mean", "mu_var", "sigma2_mean", "agg_var")):
        print("B %d L %d %s: %.3e (bound %.3e)" % (B, L, what, err[r].max(), bound[r].max()))
        assert (err[r] <= bound[r]).all(), (what, float((err[r] / bound[r]).max()))
        assert bound[r].max() <= 1e-4 * np.abs(want[r]).max() or (what in ("mu_var", "agg_var") and B == 1)
    if B == 1:
        assert (got[2] == 0).all()                              # one molecule: m^2 - m m is exact in fp64
    if L >= 8 and B >= 3:
        # the cancelling column by itself: its bound is relative to E[m^2] = 1e4 and still under 1e-4 of its own variance
        print("B %d L %d cancelling column: mu_var %.6e, error %.3e (bound %.3e)" % (B, L, want[2, CANCEL], err[2, CANCEL],
                                                                                  bound[2, CANCEL]))
        assert 1e-6 < want[2, CANCEL] < 1e-3 and bound[2, CANCEL] <= 1e-4 * want[2, CANCEL]
    if B >= 3:
        assert not D.kl_dim(mean, pv)[B - 1, zero_cols(L)].any()
    again, _ = finish(accumulate([(mean, pv)], L), L, 0.01)
    assert np.array_equal(again, got)                           # run to run


def test_batch_by_batch_is_the_whole():
    """300 molecules in one call and in three calls of 1 + 64 + 235: the accumulators agree within the fp64 bound (relative to
    the sums of the addends' magnitudes), the finished statistics within that plus the one fp32 rounding each of them took"""
    B, L = 300, 8
    mean, pv, _ = case(B, L)
    cuts = [(mean[:1], pv[:1]), (mean[1:65], pv[1:65]), (mean[65:], pv[65:])]
    one, three = accumulate([(mean, pv)], L), accumulate(cuts, L)
    m = mean.astype(np.float64)
    scale = np.stack([np.full(L, float(B)), np.abs(m).sum(axis=0), (m * m).sum(axis=0), np.exp(-np.abs(pv.astype(np.float64))).sum(axis=0),
                      np.abs(D.kl_dim(mean, pv)).sum(axis=0)])
    a, b = f64(one[:5 * L]).reshape(5, L), f64(three[:5 * L]).reshape(5, L)
    d = np.abs(a - b) / scale
    print("accumulators, one call against three: %.3e of the addends (bound %.3e)" % (d.max(), 2 * fp64(B)))
    assert (d <= 2 * fp64(B)).all() and np.array_equal(a[0], b[0])
    o1, n1 = finish(one, L, 0.01)
    o3, n3 = finish(three, L, 0.01)
    want, _ = D.finish(D.accumulate(mean, pv), 0.01)
    tol = 2 * 4 * fp64(B) * np.stack([scale[4], scale[1], scale[2], scale[3], scale[2] + scale[3]]) / B + 2 * U * np.abs(want)
    e = np.abs(o1.astype(np.float64) - o3.astype(np.float64))
    print("statistics, one call against three: %.3e (bound %.3e)" % (e.max(), tol.max()))
    assert (e <= tol).all() and n1 == n3
    # two identical sequences: bit-equal
    again = accumulate(cuts, L)
    assert torch.equal(again, three)
    assert np.array_equal(finish(again, L, 0.01)[0], o3)


def test_active_units_are_counted_against_the_threshold():
    B, L = 300, 8
    mean, pv, _ = case(B, L)
    want, _ = D.finish(D.accumulate(mean, pv), 0.0)
    v = np.sort(want[2])
    gaps = (v[1:] - v[:-1]) / v[1:]
    i = int(np.argmax(gaps))
    thr = float(np.float32(0.5 * (v[i] + v[i + 1])))
    assert (np.abs(want[2] - thr) >= 1e-3 * np.maximum(want[2], thr)).all()      # on the oracle: no column near the threshold
    assert 1e-4 * want[2].max() >= stat_bounds(mean, pv, want)[2].max()          # ... and the kernel's error is far below that
    acc = accumulate([(mean, pv)], L)
    for t, n in ((thr, L - 1 - i), (0.0, L), (float(np.float32(2 * v[-1])), 0)):
        assert D.finish(D.accumulate(mean, pv), t)[1] == n
        out, got = finish(acc, L, t)
        assert got == n and got == int((out[2] > np.float32(t)).sum())
    # through the wrapper
    out, na = F_.latent_dim_finish(acc[:5 * L].reshape(5, L), thr)
    assert na.dtype == torch.int32 and int(na) == L - 1 - i and out.shape == (5, L)


@pytest.mark.parametrize("L", [1, 65])
def test_nothing_accumulated_gives_zeros(L):
    acc = torch.full((5 * L + 4,), SENT, dtype=torch.float64, device=DEV)
    acc[:5 * L] = 0.0
    out, n = finish(acc, L, 0.01)
    assert not out.any() and n == 0
    out, n = finish(acc, L, -1.0)                                # not even under a negative threshold: N = 0 is inactive
    assert not out.any() and n == 0


# ---------------------------------------------------------------------------------------------- free bits
def lambdas(kb):
    """0, a midpoint between the two neighbouring klbar_j that lie farthest apart (relative), a value above every klbar_j"""
    out = [("zero", 0.0)]
    s = np.sort(kb)
    if len(s) > 1:
        i = int(np.argmax((s[1:] - s[:-1]) / np.maximum(s[1:], 1e-300)))
        mid = float(np.float32(0.5 * (s[i] + s[i + 1])))
        assert abs(mid - s[i]) >= 1e-3 * mid and abs(s[i + 1] - mid) >= 1e-3 * s[i + 1]
        out.append(("mid", mid))
    out.append(("above", float(np.float32(2 * s[-1] + 1))))
    return out


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_free_bits_forward_and_backward_equal_fp64(B, L):
    mean, pv, w_ = case(B, L)
    worst = {}
    for w in (None, w_):
        kb = D.klbar(mean, pv, w)
        for name, lam in lambdas(kb):
            assert (np.abs(kb - lam) >= 1e-3 * np.maximum(kb, lam))[kb != lam].all() and (lam > 0 or (kb >= 0).all())
            want_kd, want_term = D.free_bits_kl(mean, pv, w, lam)
            kd, term = free_bits(mean, pv, w, lam)
            bk = klbar_bound(mean, pv, w)
            ek = np.abs(kd.astype(np.float64) - want_kd)
            assert (ek <= bk).all(), ("kl_dims", name, float((ek / bk).max()))
            assert bk.max() <= 1e-4 * np.abs(want_kd).max()
            open_ = want_kd > lam
            bt = ((klbar_bound(mean, pv, w, final=False) * open_).sum() + fp64(L) * np.maximum(lam, want_kd).sum()
                  + U * abs(want_term)) * SLACK
            et = abs(float(term[0]) - want_term)
            assert et <= bt, ("term", name, et, bt)
            assert bt <= 1e-4 * abs(want_term) or want_term == 0
            if name == "above":
                # every column free: term = L lambda to one rounding (L lambda is exact in fp64 up to fp64(L))
                assert et <= (U + fp64(L)) * L * lam * SLACK
            k = worst.setdefault("fwd", [0.0, 0.0, 0.0, 0.0])
            worst["fwd"] = [max(k[0], ek.max()), max(k[1], bk.max()), max(k[2], et), max(k[3], bt)]
            for g in (None, 0.6):
                gg = 1.0 if g is None else float(np.float32(g))
                wm, wp = D.free_bits_kl_backward(mean, pv, w, lam, gg)
                dm, dp = free_bits_backward(mean, pv, w, lam, g, None)
                dm2, dp2 = free_bits_backward(mean, pv, w, lam, g, kd)
                assert np.array_equal(dm, dm2) and np.array_equal(dp, dp2)           # with and without the forward's kl_dims
                ww = np.ones(B) if w is None else w.astype(np.float64)
                c = np.where(open_[None, :], gg * ww[:, None] / B, 0.0)
                bm = (U * SLACK + 4 * E64) * np.abs(wm)
                bp = np.abs(c) * U * np.exp(-np.abs(pv.astype(np.float64))) * SLACK + (U * SLACK + 4 * E64) * np.abs(wp)
                em, ep = np.abs(dm - wm), np.abs(dp - wp)
                assert (em <= bm).all() and (ep <= bp).all(), (name, g, float(em.max()), float(ep.max()))
                # the gate of every column is the forward's (and the oracle's): a free column is exactly zero, an open one is not
                assert not dm[:, ~open_].any() and not dp[:, ~open_].any()
                for j in np.nonzero(open_)[0]:
                    assert dm[:, j].any() or not wm[:, j].any()
                assert (dp[pv == 0] == 0).all()
                if B >= 3:
                    assert not dm[B - 1, zero_cols(L)].any() and not dp[B - 1, zero_cols(L)].any()       # the exact-zero row
                if open_.any() and wm.any():
                    assert bm.max() <= 1e-4 * np.abs(wm).max() and (bp.max() <= 1e-4 * np.abs(wp).max() or not wp.any())
                if name == "above":
                    assert not dm.any() and not dp.any()
                k = worst.setdefault("bwd", [0.0, 0.0, 0.0, 0.0])
                worst["bwd"] = [max(k[0], em.max()), max(k[1], bm.max()), max(k[2], ep.max()), max(k[3], bp.max())]
            # run to run
            kd2, term2 = free_bits(mean, pv, w, lam)
            assert np.array_equal(kd, kd2) and np.array_equal(term, term2)
    print("B %d L %d: kl_dims %.3e (bound %.3e), term %.3e (%.3e); dmean %.3e (%.3e), dpre_var %.3e (%.3e)"
          % tuple([B, L] + worst["fwd"] + worst["bwd"]))


def test_a_tie_in_fp32_is_decided_by_the_fp64_sum_on_both_routes():
    """lambda = the forward's own rounded kl_dims[j]: the rounded value decides nothing there, and the backward with and
    without the forward's kl_dims must still agree -- column j is either free (all zeros) or open like its neighbours"""
    mean, pv, w = case(65, 8)
    kd, _ = free_bits(mean, pv, w, 0.0)
    for j in (0, 5):
        lam = float(kd[j])
        kd_l, _ = free_bits(mean, pv, w, lam)
        assert np.array_equal(kd_l, kd)
        a = free_bits_backward(mean, pv, w, lam, None, None)
        b = free_bits_backward(mean, pv, w, lam, None, kd)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        ref = free_bits_backward(mean, pv, w, 0.0, None, None)
        for c in range(8):
            if kd[c] > kd[j]:
                assert np.array_equal(a[0][:, c], ref[0][:, c])
            elif kd[c] < kd[j]:
                assert not a[0][:, c].any() and not a[1][:, c].any()
        assert not a[0][:, j].any() or np.array_equal(a[0][:, j], ref[0][:, j])


def test_all_zero_input_is_exactly_zero():
    z = np.zeros((1, 8), np.float32)
    kd, term = free_bits(z, z, None, 0.0)
    assert not kd.any() and term[0] == 0
    dm, dp = free_bits_backward(z, z, None, 0.0, None, None)
    assert not dm.any() and not dp.any()
    out, n = finish(accumulate([(z, z)], 8), 8, 0.01)
    assert not out[[0, 1, 2]].any() and (out[3] == 1).all() and (out[4] == 1).all() and n == 0


def test_wrappers_run_the_same_kernels():
    mean, pv, w = case(65, 8)
    lam = lambdas(D.klbar(mean, pv, w))[1][1]
    kd, term = F_.free_bits_kl(dev(mean), dev(pv), dev(w), lam)
    rk, rt = free_bits(mean, pv, w, lam)
    assert np.array_equal(kd.cpu().numpy(), rk) and np.array_equal(term.cpu().numpy(), rt)
    dm, dp = F_.free_bits_kl_backward(dev(mean), dev(pv), dev(w), lam, torch.tensor([0.6], device=DEV), kd)
    rm, rp = free_bits_backward(mean, pv, w, lam, 0.6, rk)
    assert np.array_equal(dm.cpu().numpy(), rm) and np.array_equal(dp.cpu().numpy(), rp)
    acc = torch.zeros(5, 8, dtype=torch.float64, device=DEV)
    assert F_.latent_dim_accumulate(dev(mean), dev(pv), acc) is acc
    assert torch.equal(acc.reshape(-1), accumulate([(mean, pv)], 8)[:40])
    for bad in (lambda: F_.free_bits_kl(dev(mean), dev(pv[:, :4]), None, 0.1), lambda: F_.free_bits_kl(dev(mean), dev(pv), dev(w[:3]), 0.1),
                lambda: F_.free_bits_kl(dev(mean), dev(pv), None, -0.1), lambda: F_.free_bits_kl(dev(mean), dev(pv), None, float("nan")),
                lambda: F_.latent_dim_accumulate(dev(mean), dev(pv), torch.zeros(5, 9, dtype=torch.float64, device=DEV)),
                lambda: F_.latent_dim_accumulate(dev(mean), dev(pv), torch.zeros(5, 8, device=DEV)),
                lambda: F_.latent_dim_finish(torch.zeros(4, 8, dtype=torch.float64, device=DEV)),
                lambda: F_.free_bits_kl_backward(dev(mean), dev(pv), None, 0.1, None, kd[:4])):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_are_refused_before_any_launch():
    lib, s = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    d = torch.full((64,), SENT, dtype=torch.float64, device=DEV)
    n = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    nan = float("nan")
    big = F_.FREE_BITS_MAX_L + 1
    acc = lib.ggpm_latent_dim_accumulate
    assert acc(None, P(f), 3, 8, P(d), s) == ERR_ARG and acc(P(f), None, 3, 8, P(d), s) == ERR_ARG
    assert acc(P(f), P(f), 3, 8, None, s) == ERR_ARG
    assert acc(P(f), P(f), 0, 8, P(d), s) == ERR_ARG and acc(P(f), P(f), 3, 0, P(d), s) == ERR_ARG
    assert acc(P(f), P(f), -1, 8, P(d), s) == ERR_ARG
    fin = lib.ggpm_latent_dim_finish
    assert fin(None, 8, 0.01, P(f), P(n), s) == ERR_ARG and fin(P(d), 8, 0.01, None, P(n), s) == ERR_ARG
    assert fin(P(d), 8, 0.01, P(f), None, s) == ERR_ARG and fin(P(d), 0, 0.01, P(f), P(n), s) == ERR_ARG
    assert fin(P(d), 8, nan, P(f), P(n), s) == ERR_ARG
    fb = lambda **kw: lib.ggpm_free_bits_kl(*[kw.get(k, v) for k, v in (
        ("mean", P(f)), ("pv", P(f)), ("w", None), ("B", 3), ("L", 8), ("lam", 0.5), ("kl_dims", P(f)), ("term", P(f)))], s)
    assert fb(mean=None) == ERR_ARG and fb(pv=None) == ERR_ARG and fb(kl_dims=None) == ERR_ARG and fb(term=None) == ERR_ARG
    assert fb(B=0) == ERR_ARG and fb(L=0) == ERR_ARG and fb(L=big, B=1) == ERR_ARG
    assert fb(lam=-0.5) == ERR_ARG and fb(lam=nan) == ERR_ARG
    bw = lambda **kw: lib.ggpm_free_bits_kl_backward(*[kw.get(k, v) for k, v in (
        ("mean", P(f)), ("pv", P(f)), ("w", None), ("gate", None), ("B", 3), ("L", 8), ("lam", 0.5), ("g", None),
        ("dmean", P(f)), ("dpv", P(f)))], s)
    assert bw(mean=None) == ERR_ARG and bw(pv=None) == ERR_ARG and bw(dmean=None) == ERR_ARG and bw(dpv=None) == ERR_ARG
    assert bw(B=0) == ERR_ARG and bw(L=0) == ERR_ARG and bw(L=big, B=1) == ERR_ARG
    assert bw(lam=-0.5) == ERR_ARG and bw(lam=nan) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all() and (d.cpu().numpy() == SENT).all() and (n.cpu().numpy() == -7).all()   # nothing ran


def test_the_widest_accepted_latent():
    """L at GGPM_FREE_BITS_MAX_L: every LDS slot of the workgroup is used, the last column included"""
    B, L = 2, F_.FREE_BITS_MAX_L
    rs = np.random.RandomState(11)
    mean, pv = rs.standard_normal((B, L)).astype(np.float32), rs.standard_normal((B, L)).astype(np.float32)
    lam = 0.25
    want_kd, want_term = D.free_bits_kl(mean, pv, None, lam)
    kd, term = free_bits(mean, pv, None, lam)
    bk = klbar_bound(mean, pv, None)
    assert (np.abs(kd - want_kd) <= bk).all()
    near = np.abs(want_kd - lam) < 1e-3 * lam                        # (columns the oracle cannot place: either side is allowed)
    bt = (klbar_bound(mean, pv, None, final=False).sum() + fp64(L) * np.maximum(lam, want_kd).sum() + U * want_term) * SLACK
    print("L %d: term %.9g, fp64 %.9g, error %.3e (bound %.3e); %d columns within 1e-3 of lambda" %
          (L, float(term[0]), want_term, abs(float(term[0]) - want_term), bt, int(near.sum())))
    assert abs(float(term[0]) - want_term) <= bt and bt <= 1e-4 * want_term
    dm, dp = free_bits_backward(mean, pv, None, lam, None, kd)
    open_ = want_kd > lam
    assert not dm[:, ~open_ & ~near].any() and dm[:, open_ & ~near].any(axis=0).all()
