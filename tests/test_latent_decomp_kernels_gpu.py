"""GPU: the three entries of csrc/latent_decomp.hip called on their own against the fp64 numpy forms of
tests/latent_decomp_oracle.py, at the smallest shapes that can break them: one draw per molecule and three; one molecule,
two (identical: p = 0.5 each), three, past one and past two wave strides of j-strided lanes; one column, a few, past one
wave of l-strided lanes (and past one 64-column tile of the backward's column pass).  Inputs: means scaled by 0.1 (heavy
overlap), pre_var of both signs and exactly 0, from three molecules on one with pre_var = -30 (its off-diagonal terms
underflow to exactly 0), a z row at 50, coef with zero entries and with a = b = c3.

Bounds.  Kernel and oracle both work in fp64 from the same fp32 inputs, so they differ by fp64 roundings and, where a fp32
value is stored, one rounding of it.  With u = 2^-24, e = 2^-52 and |x| meaning the sum of the magnitudes of the addends of x:
  * ell = -0.5 (log 2pi + lv + d^2 iv): the difference, the exponential (1 ulp), two products and two additions on either
    side:  err_ell = 8 e |ell|.
  * S = sum_l ell: L additions in either order:  err_S = (L + 40) e |S|  (the 8 e of the addends included).
  * A = logsumexp_j S: the derivative by S_j is p_j, so an error of S_j counts p_j times -- the molecule whose |S| is 1e16
    has p = 0 exactly and counts nothing; written with expm1 so that it holds for errors that are not small.  The running
    (max, sum) pairs add (B + 16) roundings of a sum of positive terms, each merged with two exponentials, then one log:
        err_A = sum_j p_j expm1(err_S_j) + (8 (B + 16) + 8) e (1 + |A|);      err_D likewise from err_ell and r.
  * mi = S_ii - A + c, tc = A - sum_l D + (L - 1) c, dwkl = sum_l D - L c - logp, dwkl_dim = D - c + (log 2pi + z^2) / 2:
    the errors of their terms + (L + 16) e |.| + u |value| for the rounding where it is stored.  The stashes lse_joint = A and
    lse_dim = D are fp64: err_A, err_D with no rounding.
  * backward: p = exp(S - A) and r = exp(ell - D) carry the relative errors expm1(err_S + err_A) and expm1(err_ell + err_D);
    G = a [i == j] + (b - a) p + (c3 - b) r then errs by |b - a| p rel_p + |c3 - b| r rel_r + 8 e |G|, and every sum of n
    addends G x by sum (dG |x| + 8 e |G x|) + (n + 16) e |sum| + u |value|.  With one molecule every logsumexp is its only
    term: A = S and D = ell bit for bit on either side, so p = r = 1 exactly and rel_p = rel_r = 0.
  * a fp32 value below the normal range rounds to within 2^-150 absolute, not u relative (a weight of 1e-217 on the molecule
    with pre_var = -30 is stored as 0): every u |value| above is u |value| + 2^-150.
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure.  The measured maxima are printed
beside the bounds.  On an MI355X, largest error / largest bound of the case where they come closest: mi 4.5e-4 / 6.4e-4, tc
6.9e-3 / 8.2e-3 (values of 1e5 on the z row at 50), dwkl 3.8e-6 / 6.0e-6, dwkl_dim 6.0e-6 / 9.0e-6, lse_joint 1.8e-15 / 5.7e-13,
lse_dim 8.9e-16 / 2.3e-13, dz 4.8e-7 / 5.9e-7, dmean 1.5e-5 / 1.7e-5, dpre_var 1.2e-7 / 1.3e-7."""
import functools

import numpy as np
import pytest
import torch

import latent_decomp_oracle as O
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
E64 = 2.0 ** -52
TINY32 = 2.0 ** -150        # half the smallest fp32 subnormal
SENT = -777.25
ERR_ARG = 1
P = F_._p
SLACK = 1.0 + 2.0 ** -10
KS, BS, LS = [1, 3], [1, 2, 3, 65, 130], [1, 8, 65]
N_DATA = 250000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(K, B, L):
    """-> dict of the inputs (fp32) and of the oracle's forward"""
    rs = np.random.RandomState(K * 100000 + B * 100 + L)
    mean = (0.1 * rs.standard_normal((B, L))).astype(np.float32)
    pv = (rs.standard_normal((B, L)) * 1.5).astype(np.float32)
    pv.reshape(-1)[::5] = 0.0                                                # pre_var exactly 0 (both signs elsewhere)
    if B >= 2:
        mean[1], pv[1] = mean[0], pv[0]                                      # two identical molecules
    if B >= 3:
        pv[B - 1] = -30.0
    z = (mean[None] + np.exp(-0.5 * np.abs(pv))[None] * rs.standard_normal((K, B, L))).astype(np.float32)
    if B >= 3:
        z[:, B - 1] = mean[B - 1]                                            # its own draws sit on its mean: everything finite
    hot = None
    if B >= 4:
        hot = (K - 1, B // 2)
    elif K > 1:
        hot = (K - 1, 0)
    if hot is not None:
        z[hot] = 50.0
    coef = rs.standard_normal((K, B, 3)).astype(np.float32)
    coef.reshape(-1)[::4] = 0.0
    c = O.log_nb(N_DATA, B)
    f = O.forward(z, mean, pv, c)
    return dict(K=K, B=B, L=L, mean=mean, pv=pv, z=z, coef=coef, c=c, f=f, hot=hot)


def fp64_errors(cs):
    """the fp64 error bounds of the docstring -> dict(ell, S, A, D) and the magnitudes"""
    if "errors" not in cs:
        cs["errors"] = _fp64_errors(cs)
    return cs["errors"]


def _fp64_errors(cs):
    K, B, L = cs["K"], cs["B"], cs["L"]
    z, m, p = cs["z"].astype(np.float64), cs["mean"].astype(np.float64), cs["pv"].astype(np.float64)
    f = cs["f"]
    lv = -np.abs(p)
    d = z[:, :, None, :] - m[None, None]
    mag_ell = 0.5 * (O.LOG_2PI + np.abs(lv)[None, None] + d * d * np.exp(-lv)[None, None])
    err_ell = 8 * E64 * mag_ell
    err_S = (L + 40) * E64 * mag_ell.sum(axis=3)
    merge = (8 * (B + 16) + 8) * E64
    err_A = (f["p"] * np.expm1(np.minimum(err_S, 50.0))).sum(axis=2) + merge * (1 + np.abs(f["A"]))
    r = np.exp(O.ell(z, m, p) - f["D"][:, :, None, :])
    err_D = (r * np.expm1(np.minimum(err_ell, 50.0))).sum(axis=2) + merge * (1 + np.abs(f["D"]))
    return dict(ell=err_ell, S=err_S, A=err_A, D=err_D, r=r, d=d, iv=np.exp(-lv)[None, None], mag_ell=mag_ell)


def forward_bounds(cs):
    """-> bounds of comps [K, B, 3], dwkl_dim [K, B, L], lse_joint, lse_dim"""
    K, B, L = cs["K"], cs["B"], cs["L"]
    f, c, e = cs["f"], cs["c"], fp64_errors(cs)
    z = cs["z"].astype(np.float64)
    ar = np.arange(B)
    sumD, absD = e["D"].sum(axis=2), np.abs(f["D"]).sum(axis=2)
    logp_mag = (0.5 * (O.LOG_2PI + z * z)).sum(axis=2)
    tail = (L + 16) * E64
    b_mi = e["S"][:, ar, ar] + e["A"] + tail * (np.abs(f["diag"]) + np.abs(f["A"]) + abs(c)) + U * np.abs(f["mi"]) + TINY32
    b_tc = e["A"] + sumD + tail * (np.abs(f["A"]) + absD + L * abs(c)) + U * np.abs(f["tc"]) + TINY32
    b_dw = sumD + tail * (absD + L * abs(c) + 2 * logp_mag) + U * np.abs(f["dwkl"]) + TINY32
    b_dd = e["D"] + 8 * E64 * (np.abs(f["D"]) + abs(c) + 0.5 * (O.LOG_2PI + z * z)) + U * np.abs(f["dwkl_dim"]) + TINY32
    return np.stack([b_mi, b_tc, b_dw], axis=-1) * SLACK, b_dd * SLACK, e["A"] * SLACK, e["D"] * SLACK


def backward_bounds(cs, coef, want):
    K, B, L = cs["K"], cs["B"], cs["L"]
    f, e = cs["f"], fp64_errors(cs)
    co = coef.astype(np.float64)
    a, b, c3 = (np.abs(co[..., 0]), np.abs(co[..., 1] - co[..., 0]), np.abs(co[..., 2] - co[..., 1]))
    rel_p = np.expm1(np.minimum(e["S"] + e["A"][:, :, None] + 4 * E64, 50.0)) * (B > 1)
    rel_r = np.expm1(np.minimum(e["ell"] + e["D"][:, :, None, :] + 4 * E64, 50.0)) * (B > 1)
    eye = np.eye(B)[None, :, :, None]
    absG = a[:, :, None, None] * eye + b[:, :, None, None] * f["p"][..., None] + c3[:, :, None, None] * e["r"]
    dG = b[:, :, None, None] * (f["p"] * rel_p)[..., None] + c3[:, :, None, None] * e["r"] * rel_r + 8 * E64 * absG
    dz_w, dm_w, dp_w = want
    z = cs["z"].astype(np.float64)
    x = np.abs(e["d"]) * e["iv"]                                             # |d iv|
    y = 0.5 + 0.5 * e["d"] * e["d"] * e["iv"]                                # |-0.5 + 0.5 d^2 iv| at most
    b_dz = ((dG + 8 * E64 * absG) * x).sum(axis=2) + (B + 16) * E64 * ((absG * x).sum(axis=2) + np.abs(co[..., 2:3] * z)) \
        + U * np.abs(dz_w) + TINY32
    n = K * B
    b_dm = ((dG + 8 * E64 * absG) * x).sum(axis=(0, 1)) + (n + 16) * E64 * (absG * x).sum(axis=(0, 1)) + U * np.abs(dm_w) + TINY32
    b_dp = ((dG + 8 * E64 * absG) * y).sum(axis=(0, 1)) + (n + 16) * E64 * (absG * y).sum(axis=(0, 1)) + U * np.abs(dp_w) + TINY32
    return b_dz * SLACK, b_dm * SLACK, b_dp * SLACK


# ---------------------------------------------------------------------------------------------- raw calls, sentinels behind
def run_forward(cs, with_optional=True):
    lib, s = _lib.load(), F_._stream()
    K, B, L = cs["K"], cs["B"], cs["L"]
    n = K * B
    comps = torch.full((n * 3 + 5,), SENT, dtype=torch.float32, device=DEV)
    dd = torch.full((n * L + 5,), SENT, dtype=torch.float32, device=DEV)
    lj = torch.full((n + 3,), SENT, dtype=torch.float64, device=DEV)
    ld = torch.full((n * L + 3,), SENT, dtype=torch.float64, device=DEV)
    z, m, p = dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"])
    opt = (P(dd), P(lj), P(ld)) if with_optional else (None, None, None)
    assert lib.ggpm_latent_decomp(P(z), P(m), P(p), K, B, L, cs["c"], P(comps), *opt, s) == 0
    c_, d_, j_, l_ = comps.cpu().numpy(), dd.cpu().numpy(), lj.cpu().numpy(), ld.cpu().numpy()
    assert (c_[n * 3:] == SENT).all() and (d_[n * L:] == SENT).all() and (j_[n:] == SENT).all() and (l_[n * L:] == SENT).all()
    if not with_optional:
        assert (d_ == SENT).all() and (j_ == SENT).all() and (l_ == SENT).all()
    return (c_[:n * 3].reshape(K, B, 3).copy(), d_[:n * L].reshape(K, B, L).copy(), j_[:n].reshape(K, B).copy(),
            l_[:n * L].reshape(K, B, L).copy())


def run_backward(cs, coef, lj, ld):
    lib, s = _lib.load(), F_._stream()
    K, B, L = cs["K"], cs["B"], cs["L"]
    dz = torch.full((K * B * L + 5,), SENT, dtype=torch.float32, device=DEV)
    dm = torch.full((B * L + 5,), SENT, dtype=torch.float32, device=DEV)
    dp = torch.full((B * L + 5,), SENT, dtype=torch.float32, device=DEV)
    z, m, p, co, a, d = dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"]), dev(coef), dev(lj), dev(ld)
    assert lib.ggpm_latent_decomp_backward(P(z), P(m), P(p), P(a), P(d), P(co), K, B, L, P(dz), P(dm), P(dp), s) == 0
    x, y, w = dz.cpu().numpy(), dm.cpu().numpy(), dp.cpu().numpy()
    assert (x[K * B * L:] == SENT).all() and (y[B * L:] == SENT).all() and (w[B * L:] == SENT).all()
    return x[:K * B * L].reshape(K, B, L).copy(), y[:B * L].reshape(B, L).copy(), w[:B * L].reshape(B, L).copy()


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
def test_forward_equals_fp64_within_the_derived_bounds(K, B, L):
    cs = case(K, B, L)
    f = cs["f"]
    if B * L >= 8:
        assert (cs["pv"] > 0).any() and (cs["pv"] < 0).any()
    assert (cs["pv"] == 0).any() or B >= 3 and L == 1
    for v in f.values():
        assert np.isfinite(v).all()
    assert cs["hot"] is None or (cs["z"][cs["hot"]] == 50).all()
    if B >= 2:
        assert np.array_equal(f["p"][:, :, 0], f["p"][:, :, 1])                  # the identical pair shares its weight
    if B == 2:
        assert (np.abs(f["p"] - 0.5) <= 4 * E64 * (1 + np.abs(f["A"]))[:, :, None]).all()      # exp(S - A): S - A rounds at |A|
    if B >= 3:
        off = np.arange(B) != B - 1
        assert (f["p"][:, off, B - 1] == 0).all() and (f["p"][:, B - 1, B - 1] > 0.999).all()     # underflow to exactly 0
    comps, dd, lj, ld = run_forward(cs)
    for a in (comps, dd, lj, ld):
        assert np.isfinite(a).all()
    b_c, b_dd, b_lj, b_ld = forward_bounds(cs)
    want = np.stack([f["mi"], f["tc"], f["dwkl"]], axis=-1)
    err = np.abs(comps.astype(np.float64) - want)
    for t, what in enumerate(("mi", "tc", "dwkl")):
        print("K %d B %d L %d %s: %.3e (bound %.3e)" % (K, B, L, what, err[..., t].max(), b_c[..., t].max()))
        assert (err[..., t] <= b_c[..., t]).all(), (what, float((err[..., t] / b_c[..., t]).max()))
        # (one column: A and D are the same logsumexp and tc is identically 0 -- there is no norm to compare with)
        assert b_c[..., t].max() <= 1e-4 * np.abs(want[..., t]).max() or (what == "tc" and L == 1)
    for what, got, ref, bound in (("dwkl_dim", dd, f["dwkl_dim"], b_dd), ("lse_joint", lj, f["A"], b_lj), ("lse_dim", ld, f["D"], b_ld)):
        e = np.abs(got.astype(np.float64) - ref)
        print("K %d B %d L %d %s: %.3e (bound %.3e)" % (K, B, L, what, e.max(), bound.max()))
        assert (e <= bound).all(), (what, float((e / bound).max()))
        assert bound.max() <= 1e-4 * np.abs(ref).max()
    # the identity, within the three bounds: mi + tc + dwkl = S_ii - logp = -logpq
    s = comps.astype(np.float64).sum(axis=-1)
    assert (np.abs(s - (f["diag"] - f["logp"])) <= b_c.sum(axis=-1)).all()
    if B == 1:
        assert (np.abs(comps[..., 0] - np.float32(cs["c"])) <= U * cs["c"] * SLACK).all()         # mi = log N
    if B == 2:
        assert (np.abs(comps[..., 0].astype(np.float64) - (cs["c"] - np.log(2.0))) <= b_c[..., 0]).all()
    # run to run, and the forward-only call writes the same comps and nothing else
    again = run_forward(cs)
    assert all(np.array_equal(x, y) for x, y in zip(again, (comps, dd, lj, ld)))
    assert np.array_equal(run_forward(cs, with_optional=False)[0], comps)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("K", KS)
def test_backward_equals_fp64_within_the_derived_bounds(K, B, L):
    cs = case(K, B, L)
    _, _, lj, ld = run_forward(cs)
    assert (cs["coef"] == 0).any()
    equal = np.repeat(cs["coef"][..., 1:2], 3, axis=-1).copy()                   # a = b = c3, zero in places
    for name, coef in (("random", cs["coef"]), ("equal", equal)):
        want = O.backward(cs["z"], cs["mean"], cs["pv"], coef)
        got = run_backward(cs, coef, lj, ld)
        bounds = backward_bounds(cs, coef, want)
        for what, g, w, b in zip(("dz", "dmean", "dpre_var"), got, want, bounds):
            assert np.isfinite(g).all() and np.isfinite(w).all()
            e = np.abs(g.astype(np.float64) - w)
            print("K %d B %d L %d %s %s: %.3e (bound %.3e)" % (K, B, L, name, what, e.max(), b.max()))
            assert (e <= b).all(), (name, what, float((e / np.maximum(b, 1e-300)).max()))
            assert b.max() <= 1e-4 * np.abs(w).max() or not w.any()
        assert (got[2][cs["pv"] == 0] == 0).all()
        if name == "equal":
            # G is exactly the diagonal: dz = a (-d_ii iv_ii) + a z, dmean = sum_k a d_ii iv_ii, to the one rounding
            z, m = cs["z"].astype(np.float64), cs["mean"].astype(np.float64)
            iv = np.exp(np.abs(cs["pv"].astype(np.float64)))
            a = coef[..., 0].astype(np.float64)[:, :, None]
            d = z - m[None]
            dz_d, dm_d = a * (-d * iv[None]) + a * z, (a * d * iv[None]).sum(axis=0)
            dp_d = -np.sign(cs["pv"]) * (a * (-0.5 + 0.5 * d * d * iv[None])).sum(axis=0)
            tiny = 16 * E64
            assert (np.abs(got[0] - dz_d) <= (U * SLACK + tiny) * (np.abs(a * d * iv[None]) + np.abs(a * z))).all()
            assert (np.abs(got[1] - dm_d) <= (U * SLACK + tiny) * np.abs(a * d * iv[None]).sum(axis=0)).all()
            assert (np.abs(got[2] - dp_d) <= (U * SLACK + tiny) * np.abs(a * (0.5 + 0.5 * d * d * iv[None])).sum(axis=0)).all()
            assert (got[0][coef[..., 0] == 0] == 0).all()                         # a zero row of coef: exactly nothing
        again = run_backward(cs, coef, lj, ld)
        assert all(np.array_equal(x, y) for x, y in zip(again, got))             # run to run


def test_accumulator_over_two_batches_with_a_read_in_between():
    lib, s = _lib.load(), F_._stream()
    L = 65
    one, two = case(3, 65, L), case(1, 130, L)
    acc = torch.full((4 + L + 3,), SENT, dtype=torch.float64, device=DEV)
    acc[:4 + L] = 0.0
    ref, mag = None, np.zeros(4 + L)
    reads = []
    for cs in (one, two):
        comps, dd, _, _ = run_forward(cs)
        c_, d_ = dev(comps), dev(dd)
        assert lib.ggpm_latent_decomp_accumulate(P(c_), P(d_), cs["K"], cs["B"], L, P(acc), s) == 0
        ref = O.accumulate(comps, dd, ref)
        mag += O.accumulate(np.abs(comps), np.abs(dd))
        reads.append(acc.cpu().numpy().copy())
    rows = 3 * 65 + 130
    for got in reads:
        assert (got[4 + L:] == SENT).all()
    first = O.accumulate(*run_forward(one)[:2])
    assert reads[0][0] == 3 * 65 and reads[1][0] == rows
    e1, e2 = np.abs(reads[0][:4 + L] - first), np.abs(reads[1][:4 + L] - ref)
    bound = 2 * (rows + 16) * E64 * mag
    print("accumulator: after one batch %.3e, after two %.3e (bound %.3e)" % (e1.max(), e2.max(), bound.max()))
    assert (e1[1:] <= bound[1:]).all() and (e2[1:] <= bound[1:]).all()
    # through the wrapper, on a fresh accumulator: the same bits
    acc2 = torch.zeros(4 + L, dtype=torch.float64, device=DEV)
    for cs in (one, two):
        comps, dd, _, _ = F_.latent_decomposition(dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"]), N_DATA)
        assert F_.latent_decomp_accumulate(comps, dd, acc2) is acc2
    assert np.array_equal(acc2.cpu().numpy(), reads[1][:4 + L])


def test_wrappers_run_the_same_kernels():
    cs = case(3, 65, 8)
    comps, dd, lj, ld = F_.latent_decomposition(dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"]), N_DATA)
    raw = run_forward(cs)
    for a, b in zip((comps, dd, lj, ld), raw):
        assert np.array_equal(a.cpu().numpy(), b)
    assert lj.dtype == torch.float64 and ld.dtype == torch.float64 and comps.shape == (3, 65, 3)
    got = F_.latent_decomposition_backward(dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"]), lj, ld, dev(cs["coef"]))
    for a, b in zip(got, run_backward(cs, cs["coef"], raw[2], raw[3])):
        assert np.array_equal(a.cpu().numpy(), b)
    with pytest.raises(ValueError):
        F_.latent_decomposition(dev(cs["z"]), dev(cs["mean"]), dev(cs["pv"]), 64)        # dataset_size < B


def test_bad_arguments_are_refused_before_any_launch():
    lib, s = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    d = torch.full((4096,), SENT, dtype=torch.float64, device=DEV)
    bigK, bigB, bigL = F_.LIKELIHOOD_MAX_K + 1, F_.LATENT_DECOMP_MAX_B + 1, F_.FREE_BITS_MAX_L + 1
    fw = lambda **kw: lib.ggpm_latent_decomp(*[kw.get(k, v) for k, v in (
        ("z", P(f)), ("mean", P(f)), ("pv", P(f)), ("K", 2), ("B", 3), ("L", 8), ("c", 5.0), ("comps", P(f)), ("dd", P(f)),
        ("lj", P(d)), ("ld", P(d)))], s)
    assert fw(z=None) == ERR_ARG and fw(mean=None) == ERR_ARG and fw(pv=None) == ERR_ARG and fw(comps=None) == ERR_ARG
    assert fw(K=0) == ERR_ARG and fw(B=0) == ERR_ARG and fw(L=0) == ERR_ARG and fw(K=-1) == ERR_ARG
    assert fw(K=bigK, B=1, L=1) == ERR_ARG and fw(K=1, B=bigB, L=1) == ERR_ARG and fw(K=1, B=1, L=bigL) == ERR_ARG
    assert fw(K=1024, B=4096, L=512) == ERR_ARG                                    # K B L = 2^31, each within its own limit
    assert fw(c=float("nan")) == ERR_ARG and fw(c=float("inf")) == ERR_ARG and fw(c=-float("inf")) == ERR_ARG
    bw = lambda **kw: lib.ggpm_latent_decomp_backward(*[kw.get(k, v) for k, v in (
        ("z", P(f)), ("mean", P(f)), ("pv", P(f)), ("lj", P(d)), ("ld", P(d)), ("coef", P(f)), ("K", 2), ("B", 3), ("L", 8),
        ("dz", P(f)), ("dmean", P(f)), ("dpv", P(f)))], s)
    for k in ("z", "mean", "pv", "lj", "ld", "coef", "dz", "dmean", "dpv"):
        assert bw(**{k: None}) == ERR_ARG, k
    assert bw(K=0) == ERR_ARG and bw(B=0) == ERR_ARG and bw(L=0) == ERR_ARG
    assert bw(K=bigK, B=1, L=1) == ERR_ARG and bw(K=1, B=bigB, L=1) == ERR_ARG and bw(K=1, B=1, L=bigL) == ERR_ARG
    assert bw(K=1024, B=4096, L=512) == ERR_ARG
    ac = lambda **kw: lib.ggpm_latent_decomp_accumulate(*[kw.get(k, v) for k, v in (
        ("comps", P(f)), ("dd", P(f)), ("K", 2), ("B", 3), ("L", 8), ("acc", P(d)))], s)
    assert ac(comps=None) == ERR_ARG and ac(dd=None) == ERR_ARG and ac(acc=None) == ERR_ARG
    assert ac(K=0) == ERR_ARG and ac(B=0) == ERR_ARG and ac(L=0) == ERR_ARG
    assert ac(K=bigK, B=1, L=1) == ERR_ARG and ac(K=1, B=bigB, L=1) == ERR_ARG and ac(K=1, B=1, L=bigL) == ERR_ARG
    assert ac(K=1024, B=4096, L=512) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all() and (d.cpu().numpy() == SENT).all()      # nothing ran
