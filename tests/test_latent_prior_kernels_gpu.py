"""GPU: the three entries of csrc/latent_prior.hip called on their own against the fp64 numpy forms of
tests/latent_prior_oracle.py, at the smallest shapes that can break them.  The geometry strides the components by 4 (waves),
64 (lanes) and 256 (threads), the columns by 4 (waves) and 64 (lanes, and the 64-column tiles of the column pass) and the rows
by 4 (the waves of the column pass, which is not chunked any further): R, C and L are each taken at 1, 3, 65 and 130 -- C also
at 257 -- with the other two small, then together; L = 24 is included.  Inputs: means scaled by 0.1 (heavy overlap) and by 5
(separated); log_vars of both signs, exactly 0 and +10, and from four components on one whole component at -30 with a row of z
on its mean; one logit at -1e4 (its weight is exactly 0 in fp64); two identical components; a z row at 50; g with zero entries.

Bounds.  Kernel and oracle both work in fp64 from the same fp32 inputs, so they differ by fp64 roundings and, where a fp32
value is stored, one rounding of it.  With u = 2^-24, e = 2^-52 and |x| meaning the sum of the magnitudes of the addends of x:
  * t = log 2pi + s + d^2 exp(-s): the difference, the exponential (1 ulp), two products and two additions on either side:
    err_t = 8 e |t|;  Q = sum_j t in either order: err_Q = (L + 40) e |Q|  (the 8 e of the addends included).
  * log pi_c = a_c - logsumexp a: the running (max, sum) pairs add (C + 16) roundings of a sum of positive terms, each merged
    with two exponentials, then one log and the difference:  err_pi = (8 (C + 16) + 8) e (1 + |a_c| + |logsumexp a|).
  * comp = log pi - Q / 2:  err_comp = err_pi + err_Q / 2 + 4 e |comp|.
  * logp = logsumexp_c comp: the derivative by comp_c is gamma_c, so an error of comp_c counts gamma_c times (written with
    expm1 so that it holds for errors that are not small), then the merges:
        err_logp = sum_c gamma_c expm1(err_comp_c) + (8 (C + 16) + 8) e (1 + |logp|);
    logn = -sum_j (log 2pi + z^2) / 2: err_logn = (L + 40) e |logn|.  The stashes are fp64: err_comp, err_logp, no rounding.
  * logp as stored: err_logp + u |logp|;  ratio = logp - logn: err_logp + err_logn + 4 e (|logp| + |logn|) + u |ratio|.
  * gamma = exp(comp - logp) carries the relative error rel = expm1(err_comp + err_logp + 2 e |comp - logp|) + 4 e; with one
    component comp = logp bit for bit on either side and gamma = 1 exactly.  resp: gamma rel + u gamma.
  * backward: every sum of n addends w x with w = g gamma by sum (|w| rel |x| + 8 e |w x|) + (n + 16) e |sum| + u |value|;
    in dlogits the weight pi_c = exp(log pi_c) carries expm1(err_pi) + 4 e instead.
  * a fp32 value below the normal range rounds to within 2^-150 absolute, not u relative: every u |value| above is
    u |value| + 2^-150.
  * sampler: sd = expf(s / 2) is within one ulp (2 u sd; s / 2 is exact), the fma rounds once:
        |out - (m + exp(s / 2) n)| <= 2 u sd |n| + u |out|   with n ggpm_sample_normal's fp32 value.
    The components are integers: equal to the oracle's wherever u * total is not within 1e-9 total of a prefix sum, which the
    test asserts of every row (no case is excluded); on two equal logits every boundary is exactly representable and the
    components must be equal there too.
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure.  The measured maxima are printed
beside the bounds.  On an MI355X, largest error / largest bound of the case where they come closest: logp 1.7e-3 / 2.1e-3 and
ratio 7.1e-3 / 7.9e-3 (values of 1e4 and 1e5 on the z row at 50), resp 2.9e-8 / 6.4e-8, comp_stash 1.9e2 / 8.8e3 (values of
1e18: the z row at 50 under the component at -30), logp_stash 3.6e-15 / 8.3e-13, dz 3.7e-6 / 4.5e-6, dmeans 3.7e-6 / 4.5e-6,
dlog_vars 2.8e-5 / 3.2e-5, dlogits 5.3e-8 / 8.5e-8, sampler 4.0e-5 / 9.6e-5 (element by element at most 0.995 of its bound)."""
import functools

import numpy as np
import pytest
import torch

import latent_prior_oracle as O
import sample_oracle as S
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
E64 = 2.0 ** -52
TINY32 = 2.0 ** -150        # half the smallest fp32 subnormal
SENT = -777.25
ISENT = -77
ERR_ARG = 1
P = F_._p
SLACK = 1.0 + 2.0 ** -10
SIZES = [1, 3, 65, 130]
SHAPES = sorted(set([(R, 3, 8) for R in SIZES] + [(3, C, 8) for C in SIZES + [257]] + [(3, 3, L) for L in SIZES + [24]] +
                    [(65, 65, 24), (130, 130, 65), (5, 257, 130), (130, 1, 24), (1, 130, 1), (9, 4, 24)]))
SCALES = [0.1, 5.0]
SEED = 0x1234567890ABCDEF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(R, C, L, scale):
    """-> dict of the inputs (fp32) and of the oracle's forward"""
    rs = np.random.RandomState(R * 1000000 + C * 1000 + L + int(scale * 10) * 7919)
    a = rs.standard_normal(C).astype(np.float32)
    m = (scale * rs.standard_normal((C, L))).astype(np.float32)
    s = (1.5 * rs.standard_normal((C, L))).astype(np.float32)
    s.reshape(-1)[::5] = 0.0                                                 # log_vars exactly 0 (both signs elsewhere)
    s.reshape(-1)[3::7] = 10.0
    if C >= 2:
        a[1], m[1], s[1] = a[0], m[0], s[0]                                  # two identical components
    if C >= 3:
        a[2], m[2], s[2] = -1e4, m[0], s[0]                                  # a weight of exactly 0, beside a twin that has one
    if C >= 4:
        s[C - 1] = -30.0
    own = rs.randint(0, C, size=R)
    if C >= 3:
        own[own == 2] = 0
    if C >= 4 and R >= 3:
        own[0] = C - 1
    z = (m[own] + np.exp(0.5 * s[own]) * rs.standard_normal((R, L))).astype(np.float32)
    if C >= 4:
        z[own == C - 1] = m[C - 1]                                           # on the narrow component's mean: everything finite
    hot = R - 1 if R >= 2 else None
    if hot is not None:
        z[hot] = 50.0
    g = rs.standard_normal(R).astype(np.float32)
    g[::3] = 0.0
    return dict(R=R, C=C, L=L, a=a, m=m, s=s, z=z, g=g, hot=hot, own=own, f=O.forward(z, a, m, s))


def fp64_errors(cs):
    if "errors" not in cs:
        cs["errors"] = _fp64_errors(cs)
    return cs["errors"]


def _fp64_errors(cs):
    R, C, L, f = cs["R"], cs["C"], cs["L"], cs["f"]
    z, a, m, s = [cs[k].astype(np.float64) for k in ("z", "a", "m", "s")]
    d = z[:, None, :] - m[None]
    iv = np.exp(-s)[None]
    mag_t = O.LOG_2PI + np.abs(s)[None] + d * d * iv                         # [R, C, L]
    err_Q = (L + 40) * E64 * mag_t.sum(axis=2)
    merge = (8 * (C + 16) + 8) * E64
    lse_a = O.logsumexp(a, 0)
    err_pi = merge * (1 + np.abs(a) + abs(lse_a))                            # [C]
    mag_comp = np.abs(O.log_pi(a))[None] + 0.5 * mag_t.sum(axis=2)
    err_comp = err_pi[None] + 0.5 * err_Q + 4 * E64 * mag_comp
    err_logp = (f["resp"] * np.expm1(np.minimum(err_comp, 50.0))).sum(axis=1) + merge * (1 + np.abs(f["logp"]))
    mag_logn = 0.5 * (O.LOG_2PI + z * z).sum(axis=1)
    err_logn = (L + 40) * E64 * mag_logn
    x = np.abs(f["comp"] - f["logp"][:, None])
    rel = (np.expm1(np.minimum(err_comp + err_logp[:, None] + 2 * E64 * x, 50.0)) + 4 * E64) * (C > 1)
    return dict(comp=err_comp, logp=err_logp, logn=err_logn, mag_logn=mag_logn, rel=rel, pi=err_pi, d=d, iv=iv)


def forward_bounds(cs):
    """-> bounds of logp, ratio, resp, comp_stash, logp_stash"""
    f, e = cs["f"], fp64_errors(cs)
    b_logp = e["logp"] + U * np.abs(f["logp"]) + TINY32
    b_ratio = e["logp"] + e["logn"] + 4 * E64 * (np.abs(f["logp"]) + e["mag_logn"]) + U * np.abs(f["ratio"]) + TINY32
    b_resp = f["resp"] * e["rel"] + U * f["resp"] + TINY32
    return [b * SLACK for b in (b_logp, b_ratio, b_resp, e["comp"], e["logp"])]


def backward_bounds(cs, g, on_logp, want):
    R, C, L, f, e = cs["R"], cs["C"], cs["L"], cs["f"], fp64_errors(cs)
    z, a = cs["z"].astype(np.float64), cs["a"].astype(np.float64)
    ag = np.abs(g.astype(np.float64))
    gam, rel = f["resp"], e["rel"]
    x = np.abs(e["d"]) * e["iv"]                                             # |d iv|          [R, C, L]
    y = 0.5 * (e["d"] * e["d"] * e["iv"] + 1.0)                              # |0.5 (d^2 iv - 1)| at most
    wr = (gam * (rel + 8 * E64))[:, :, None]                                 # the error of gamma x, per unit |x|
    dz_w, dm_w, ds_w, da_w = want
    b_dz = ag[:, None] * ((wr * x).sum(axis=1) + (C + 16) * E64 * ((gam[:, :, None] * x).sum(axis=1) + np.abs(z))) \
        + U * np.abs(dz_w) + TINY32
    gw = ag[:, None, None]
    b_dm = (gw * wr * x).sum(axis=0) + (R + 16) * E64 * (gw * gam[:, :, None] * x).sum(axis=0) + U * np.abs(dm_w) + TINY32
    b_ds = (gw * wr * y).sum(axis=0) + (R + 16) * E64 * (gw * gam[:, :, None] * y).sum(axis=0) + U * np.abs(ds_w) + TINY32
    pi = np.exp(O.log_pi(a))
    dpi = pi * (np.expm1(e["pi"]) + 4 * E64)
    b_da = (ag[:, None] * (gam * rel + dpi[None] + 8 * E64 * (gam + pi[None]))).sum(axis=0) \
        + (R + 16) * E64 * (ag[:, None] * (gam + pi[None])).sum(axis=0) + U * np.abs(da_w) + TINY32
    return [b * SLACK for b in (b_dz, b_dm, b_ds, b_da)]


# ---------------------------------------------------------------------------------------------- raw calls, sentinels behind
def run_forward(cs, with_optional=True):
    lib, st = _lib.load(), F_._stream()
    R, C, L = cs["R"], cs["C"], cs["L"]
    logp = torch.full((R + 5,), SENT, dtype=torch.float32, device=DEV)
    ratio = torch.full((R + 5,), SENT, dtype=torch.float32, device=DEV)
    resp = torch.full((R * C + 5,), SENT, dtype=torch.float32, device=DEV)
    comp = torch.full((R * C + 3,), SENT, dtype=torch.float64, device=DEV)
    lps = torch.full((R + 3,), SENT, dtype=torch.float64, device=DEV)
    z, a, m, s = dev(cs["z"]), dev(cs["a"]), dev(cs["m"]), dev(cs["s"])
    opt = (P(resp), P(comp), P(lps)) if with_optional else (None, None, None)
    assert lib.ggpm_mixture_logp(P(z), P(a), P(m), P(s), R, C, L, P(logp), P(ratio), *opt, st) == 0
    out = [t.cpu().numpy() for t in (logp, ratio, resp, comp, lps)]
    for o, n in zip(out, (R, R, R * C, R * C, R)):
        assert (o[n:] == SENT).all()
    if not with_optional:
        assert all((o == SENT).all() for o in out[2:])
    return (out[0][:R].copy(), out[1][:R].copy(), out[2][:R * C].reshape(R, C).copy(), out[3][:R * C].reshape(R, C).copy(),
            out[4][:R].copy())


def run_backward(cs, g, on_logp, comp, lps, want_dz=True, want_params=True):
    lib, st = _lib.load(), F_._stream()
    R, C, L = cs["R"], cs["C"], cs["L"]
    outs = [torch.full((n + 5,), SENT, dtype=torch.float32, device=DEV) for n in (R * L, C * L, C * L, C)]
    z, a, m, s, g_, c_, l_ = dev(cs["z"]), dev(cs["a"]), dev(cs["m"]), dev(cs["s"]), dev(g), dev(comp), dev(lps)
    ptrs = [P(outs[0]) if want_dz else None] + [P(t) if want_params else None for t in outs[1:]]
    assert lib.ggpm_mixture_logp_backward(P(z), P(a), P(m), P(s), P(c_), P(l_), P(g_), int(on_logp), R, C, L, *ptrs, st) == 0
    got = [t.cpu().numpy() for t in outs]
    for o, n in zip(got, (R * L, C * L, C * L, C)):
        assert (o[n:] == SENT).all()
    if not want_dz:
        assert (got[0] == SENT).all()
    if not want_params:
        assert all((o == SENT).all() for o in got[1:])
    return (got[0][:R * L].reshape(R, L).copy(), got[1][:C * L].reshape(C, L).copy(), got[2][:C * L].reshape(C, L).copy(),
            got[3][:C].copy())


def run_sampler(a, m, s, ids, seed=SEED, ld=None, with_comp=True):
    lib, st = _lib.load(), F_._stream()
    (C, L), rows = m.shape, len(ids)
    ld = L if ld is None else ld
    out = torch.full((rows * ld + 5,), SENT, dtype=torch.float32, device=DEV)
    comp = torch.full((rows + 3,), ISENT, dtype=torch.int32, device=DEV)
    lo, hi = S.split(seed)
    assert lib.ggpm_sample_mixture(P(dev(a)), P(dev(m)), P(dev(s)), C, P(out), rows, L, ld, P(dev(np.asarray(ids, np.int32))), lo, hi,
                                   P(comp) if with_comp else None, st) == 0
    o, c = out.cpu().numpy(), comp.cpu().numpy()
    assert (o[rows * ld:] == SENT).all() and (c[rows:] == ISENT).all()
    o = o[:rows * ld].reshape(rows, ld)
    assert (o[:, L:] == SENT).all()                                          # the pad columns are left alone
    if not with_comp:
        assert (c == ISENT).all()
    return o[:, :L].copy(), c[:rows].copy()


def normals(ids, L, seed=SEED):
    lo, hi = S.split(seed)
    return F_.sample_normal(len(ids), L, lo, hi, ids=np.asarray(ids, np.int64), device=DEV).cpu().numpy()


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("R,C,L", SHAPES)
def test_forward_equals_fp64_within_the_derived_bounds(R, C, L, scale):
    cs = case(R, C, L, scale)
    f = cs["f"]
    for v in f.values():
        assert np.isfinite(v).all()
    assert cs["hot"] is None or (cs["z"][cs["hot"]] == 50).all()
    if C * L >= 24:
        assert (cs["s"] > 0).any() and (cs["s"] < 0).any() and (cs["s"] == 0).any() and (cs["s"] == 10).any()
    if C >= 2:
        assert np.array_equal(f["resp"][:, 0], f["resp"][:, 1])                  # the identical pair shares its weight
    if C >= 3:
        assert (f["resp"][:, 2] == 0).all() and np.exp(O.log_pi(cs["a"]))[2] == 0    # the logit at -1e4: exactly nothing
    if C >= 4:
        assert (cs["s"][C - 1] == -30).all()
        on = cs["own"] == C - 1
        if cs["hot"] is not None:
            on[cs["hot"]] = False
        assert (f["resp"][~on, C - 1] == 0).all() and (R < 3 or (f["resp"][on, C - 1] > 0.999).all() and on.any())
    got = run_forward(cs)
    for x in got:
        assert np.isfinite(x).all()
    want = (f["logp"], f["ratio"], f["resp"], f["comp"], f["logp"])
    for what, x, w, b in zip(("logp", "ratio", "resp", "comp_stash", "logp_stash"), got, want, forward_bounds(cs)):
        err = np.abs(x.astype(np.float64) - w)
        print("R %d C %d L %d x%g %s: %.3e (bound %.3e)" % (R, C, L, scale, what, err.max(), b.max()))
        assert (err <= b).all(), (what, float((err / b).max()))
        assert b.max() <= 1e-4 * np.abs(w).max()
    if C == 1:
        assert (got[2] == 1.0).all()
    # run to run, and the forward-only call writes the same logp and ratio and nothing else
    again = run_forward(cs)
    assert all(np.array_equal(x, y) for x, y in zip(again, got))
    bare = run_forward(cs, with_optional=False)
    assert np.array_equal(bare[0], got[0]) and np.array_equal(bare[1], got[1])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("R,C,L", SHAPES)
def test_backward_equals_fp64_within_the_derived_bounds(R, C, L, scale):
    cs = case(R, C, L, scale)
    _, _, _, comp, lps = run_forward(cs)
    g = cs["g"]
    assert (g == 0).any()
    for on_logp in (False, True):
        want = O.backward(cs["z"], cs["a"], cs["m"], cs["s"], g, on_logp)
        got = run_backward(cs, g, on_logp, comp, lps)
        for what, x, w, b in zip(("dz", "dmeans", "dlog_vars", "dlogits"), got, want, backward_bounds(cs, g, on_logp, want)):
            assert np.isfinite(x).all() and np.isfinite(w).all()
            err = np.abs(x.astype(np.float64) - w)
            print("R %d C %d L %d x%g on_logp %d %s: %.3e (bound %.3e)" % (R, C, L, scale, on_logp, what, err.max(), b.max()))
            assert (err <= b).all(), (what, on_logp, float((err / np.maximum(b, 1e-300)).max()))
            # (up to three components all that have weight are twins: gamma = pi for every row and dlogits is identically 0,
            # roundings apart -- there is no norm to compare with)
            assert b.max() <= 1e-4 * np.abs(w).max() or not w.any() or (what == "dlogits" and C <= 3)
        assert (got[0][g == 0] == 0).all()                                       # a zero g: exactly nothing for its row
        if C >= 3:
            assert (got[1][2] == 0).all() and (got[2][2] == 0).all() and got[3][2] == 0      # the weightless component
        if C == 1:
            assert (got[3] == 0).all()                                           # softmax of one logit is constant
        # the two passes on their own write the same bits and leave the other group alone
        only_z = run_backward(cs, g, on_logp, comp, lps, want_params=False)
        only_p = run_backward(cs, g, on_logp, comp, lps, want_dz=False)
        assert np.array_equal(only_z[0], got[0]) and all(np.array_equal(x, y) for x, y in zip(only_p[1:], got[1:]))
        again = run_backward(cs, g, on_logp, comp, lps)
        assert all(np.array_equal(x, y) for x, y in zip(again, got))             # run to run
    # ratio and logp differ by the standard normal's part alone
    dz_r = run_backward(cs, g, False, comp, lps, want_params=False)[0]
    dz_l = run_backward(cs, g, True, comp, lps, want_params=False)[0]
    zz = g.astype(np.float64)[:, None] * cs["z"].astype(np.float64)
    assert (np.abs(dz_r.astype(np.float64) - dz_l - zz) <= U * SLACK * (np.abs(dz_r) + np.abs(dz_l)) + 2 * TINY32).all()


def sampler_case(C, L, scale=1.0):
    rs = np.random.RandomState(C * 1000 + L)
    a = rs.standard_normal(C).astype(np.float32)
    if C >= 3:
        a[1] = -1e4
    m = (scale * rs.standard_normal((C, L))).astype(np.float32)
    s = (1.5 * rs.standard_normal((C, L))).astype(np.float32)
    s.reshape(-1)[::5] = 0.0
    s.reshape(-1)[3::7] = 10.0
    if C >= 2:
        s[C - 1] = -30.0
    return a, m, s


@pytest.mark.parametrize("L", [1, 24, 65, 130])
@pytest.mark.parametrize("C", [1, 3, 65, 130, 257])
def test_sampler_components_equal_the_oracle_and_values_stay_within_one_exp_and_one_fma(C, L):
    a, m, s = sampler_case(C, L)
    ids = np.concatenate([np.arange(120), [2 ** 31 - 1, -1, -2 ** 31, 123456789, 7, 7]]).astype(np.int64)
    want_c, margin = O.components(SEED, ids, a)
    assert margin.min() > 1e-9, margin.min()                                     # no boundary within reach of a rounding
    out, comp = run_sampler(a, m, s, ids, ld=L + 3)
    assert np.array_equal(comp, want_c)
    if C >= 3:
        assert (comp != 1).all() and len(set(comp.tolist())) >= 2
    n = normals(ids, L).astype(np.float64)
    sd = np.exp(0.5 * s.astype(np.float64))[comp]
    ref = m.astype(np.float64)[comp] + sd * n
    bound = (2 * U * sd * np.abs(n) + U * np.abs(ref) + TINY32) * SLACK
    err = np.abs(out.astype(np.float64) - ref)
    print("C %d L %d sampler: %.3e (bound %.3e, largest ratio %.3f)" % (C, L, err.max(), bound.max(), (err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    assert bound.max() <= 1e-4 * np.abs(ref).max()
    assert np.array_equal(out[-1], out[-2])                                      # one id twice: one draw
    again = run_sampler(a, m, s, ids, ld=L + 3)
    assert np.array_equal(again[0], out) and np.array_equal(again[1], comp)      # run to run
    assert np.array_equal(run_sampler(a, m, s, ids, with_comp=False)[0], out)    # dense, and without the components
    # a row drawn alone, and inside another batch in another position
    for r in (0, 57, 121):
        alone = run_sampler(a, m, s, ids[r:r + 1])
        assert np.array_equal(alone[0][0], out[r]) and alone[1][0] == comp[r]
    back = run_sampler(a, m, s, ids[::-1].copy())
    assert np.array_equal(back[0][::-1], out) and np.array_equal(back[1][::-1], comp)
    other = run_sampler(a, m, s, ids, seed=SEED + 1)
    assert not np.array_equal(other[0], out)


def test_sampler_on_two_equal_logits_splits_at_one_half_exactly():
    L = 8
    ids = np.arange(4096)
    m = np.stack([np.full(L, -3.0), np.full(L, 3.0)]).astype(np.float32)
    s = np.zeros((2, L), np.float32)
    for a in (np.zeros(2, np.float32), np.full(2, 7.5, np.float32)):
        u = O.uniforms(SEED, ids)
        out, comp = run_sampler(a, m, s, ids)
        assert np.array_equal(comp, (u >= 0.5).astype(np.int32)) and 1800 < comp.sum() < 2300
        assert np.array_equal(comp, O.components(SEED, ids, a)[0])
        assert np.array_equal(out, m[comp] + normals(ids, L))                    # expf(0) = 1: the fma adds the mean, one rounding
    # the standard one-component prior IS ggpm_sample_normal
    for L1 in (1, 24, 130):
        out, comp = run_sampler(np.zeros(1, np.float32), np.zeros((1, L1), np.float32), np.zeros((1, L1), np.float32), ids[:130])
        assert np.array_equal(out, normals(ids[:130], L1)) and not comp.any()


def test_wrappers_run_the_same_kernels():
    cs = case(65, 65, 24, 5.0)
    z, a, m, s, g = [dev(cs[k]) for k in ("z", "a", "m", "s", "g")]
    raw = run_forward(cs)
    got = F_.mixture_logp(z, a, m, s, want_resp=True)
    for x, y in zip(got, raw):
        assert np.array_equal(x.cpu().numpy(), y)
    assert got[3].dtype == torch.float64 and got[4].dtype == torch.float64
    bare = F_.mixture_logp(z, a, m, s, want_stash=False)
    assert bare[2] is None and bare[3] is None and bare[4] is None and torch.equal(bare[1], got[1])
    for on_logp in (True, False):
        back = F_.mixture_logp_backward(z, a, m, s, got[3], got[4], g, on_logp)
        for x, y in zip(back, run_backward(cs, cs["g"], on_logp, raw[3], raw[4])):
            assert np.array_equal(x.cpu().numpy(), y)
    frozen = F_.mixture_logp_backward(z, a, m, s, got[3], got[4], g, False, want_params=False)
    assert frozen[1] is None and frozen[2] is None and frozen[3] is None and torch.equal(frozen[0], back[0])
    lo, hi = S.split(SEED)
    out, comp = F_.sample_mixture(a, m, s, 130, lo, hi, want_components=True)
    r_out, r_comp = run_sampler(cs["a"], cs["m"], cs["s"], np.arange(130))
    assert np.array_equal(out.cpu().numpy(), r_out) and np.array_equal(comp.cpu().numpy(), r_comp)


def test_bad_arguments_are_refused_before_any_launch():
    lib, st = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    d = torch.full((4096,), SENT, dtype=torch.float64, device=DEV)
    i = torch.full((64,), ISENT, dtype=torch.int32, device=DEV)
    bigC, bigL = F_.MIXTURE_MAX_C + 1, F_.FREE_BITS_MAX_L + 1
    fw = lambda **kw: lib.ggpm_mixture_logp(*[kw.get(k, v) for k, v in (
        ("z", P(f)), ("a", P(f)), ("m", P(f)), ("s", P(f)), ("R", 2), ("C", 3), ("L", 8), ("logp", P(f)), ("ratio", P(f)),
        ("resp", P(f)), ("comp", P(d)), ("lps", P(d)))], st)
    for k in ("z", "a", "m", "s", "logp", "ratio"):
        assert fw(**{k: None}) == ERR_ARG, k
    assert fw(R=0) == ERR_ARG and fw(C=0) == ERR_ARG and fw(L=0) == ERR_ARG and fw(R=-1) == ERR_ARG
    assert fw(C=bigC) == ERR_ARG and fw(L=bigL) == ERR_ARG
    assert fw(R=1 << 19, L=4096) == ERR_ARG and fw(R=1 << 19, C=4096, L=1) == ERR_ARG        # R L = 2^31, R C = 2^31
    bw = lambda **kw: lib.ggpm_mixture_logp_backward(*[kw.get(k, v) for k, v in (
        ("z", P(f)), ("a", P(f)), ("m", P(f)), ("s", P(f)), ("comp", P(d)), ("lps", P(d)), ("g", P(f)), ("on_logp", 0), ("R", 2),
        ("C", 3), ("L", 8), ("dz", P(f)), ("dm", P(f)), ("ds", P(f)), ("da", P(f)))], st)
    for k in ("z", "a", "m", "s", "comp", "lps", "g"):
        assert bw(**{k: None}) == ERR_ARG, k
    for part in (("dm",), ("ds",), ("da",), ("dm", "ds"), ("ds", "da"), ("dm", "da"), ("dz", "dm", "ds", "da")):
        assert bw(**{k: None for k in part}) == ERR_ARG, part                            # the group is whole or absent
    assert bw(on_logp=2) == ERR_ARG and bw(on_logp=-1) == ERR_ARG
    assert bw(R=0) == ERR_ARG and bw(C=0) == ERR_ARG and bw(L=0) == ERR_ARG
    assert bw(C=bigC) == ERR_ARG and bw(L=bigL) == ERR_ARG and bw(R=1 << 19, L=4096) == ERR_ARG
    sm = lambda **kw: lib.ggpm_sample_mixture(*[kw.get(k, v) for k, v in (
        ("a", P(f)), ("m", P(f)), ("s", P(f)), ("C", 3), ("out", P(f)), ("rows", 2), ("cols", 8), ("ld", 8), ("ids", P(i)),
        ("lo", 1), ("hi", 2), ("comp", P(i)))], st)
    for k in ("a", "m", "s", "out", "ids"):
        assert sm(**{k: None}) == ERR_ARG, k
    assert sm(rows=0) == ERR_ARG and sm(cols=0) == ERR_ARG and sm(C=0) == ERR_ARG and sm(ld=7) == ERR_ARG
    assert sm(C=bigC) == ERR_ARG and sm(cols=bigL, ld=bigL) == ERR_ARG and sm(rows=1 << 19, cols=4096, ld=4096) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all() and (d.cpu().numpy() == SENT).all() and (i.cpu().numpy() == ISENT).all()
