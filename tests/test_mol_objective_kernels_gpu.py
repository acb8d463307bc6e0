"""GPU: the entries ``bound_loss`` adds (csrc/mol_loss.hip, csrc/motif_assm.hip) called on their own against the fp64 numpy
forms of tests/mol_objective_oracle.py, at the smallest shapes that can break them: sample counts past one wave of k-strided
lanes, row counts around one wave and one block, widths past 64 with ld > N, molecules without rows, rows of no molecule,
absent and non-uniform weights, log-weights hundreds apart, pre_var of both signs and 0.

Bounds, with u = 2^-24 (half an fp32 ulp, relative) and fp64 = what (K + 16) fp64 operations at the scale of the largest
log-weight can add (2^-52 each):
  * objective: fp32 inputs are exact, everything is formed in fp64 and rounded once -> u |ref| + fp64 |ref| for the loss and
    every coefficient (2^-150, half the smallest subnormal, where a softmax weight underflows fp32); the softmax
    coefficients of a molecule therefore sum to w / B within K of those.
  * row scaling: fl(fl(g coef) d) -> 2 u |ref| (one rounding without g); rows of no molecule are exactly 0, columns past N
    and rows past M are untouched.
  * latent backward: z is re-formed in fp32 like the forward, dz_err = u (3 |s eps| + |z|) with s = expf(lv / 2) (2u); with
    G = g c_logpq, a = dz - G z:
        dmean: sum_k |G| dz_err + u |dmean|
        dlv:   sum_k (|G| dz_err |s eps| / 2 + |a| u |s eps|) + |gk| u e^lv + u |dlv|        (expf: 2u)
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure where the shape has enough elements.
The measured maxima are printed beside the bounds."""
import functools
import os

import numpy as np
import pytest
import torch

import mol_objective_oracle as O
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT = -777.25
ERR_ARG = 1
P = F_._p
SLACK = 1.0 + 2.0 ** -10


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------- ggpm_bound_objective
def objective_case(K, B):
    rs = np.random.RandomState(K * 100 + B)
    parts = (rs.rand(K, B, 4) * 2).astype(np.float32)
    if K > 1:
        parts[:, :, 0] += np.linspace(20.0, 140.0, K).astype(np.float32)[rs.permutation(K)][:, None]    # nll spread 120 over k
    parts[:, B // 2, 3] = 0.0
    logpq = (rs.standard_normal((K, B)) * 3).astype(np.float32)
    logpq[:, 0] += 200.0
    kl = (rs.rand(B) * 4).astype(np.float32)
    w = (rs.rand(B) * 3 + 0.1).astype(np.float32)
    return parts, logpq, kl, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("objective,beta", [("elbo", 0.3), ("elbo", 1.0), ("iwae", 1.0)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 3, 65])
def test_objective_and_coefficients_equal_fp64(K, B, objective, beta, weighted):
    parts, logpq, kl, w = objective_case(K, B)
    w = w if weighted else None
    got = F_.bound_objective(dev(parts), dev(logpq), dev(kl), None if w is None else dev(w), objective, beta)
    loss, c_nll, c_logpq, c_kl = (f64(t) for t in got)
    want = O.objective(parts, logpq, kl, w, objective, float(np.float32(beta)))
    lw = logpq.astype(np.float64) - O.nll_of(parts)
    if K > 1:
        assert (lw.max(axis=0) - lw.min(axis=0)).min() > 100           # exp() of the differences underflows fp32
    fp64 = (K + 16) * 2.0 ** -52 * max(np.abs(lw).max(), 1.0)
    for g_, w_, what in ((loss.reshape(()), np.asarray(want[0]), "loss"), (c_nll, want[1], "c_nll"), (c_logpq, want[2], "c_logpq"),
                         (c_kl, want[3], "c_kl")):
        bound = (U * SLACK + fp64) * np.abs(w_) + 2.0 ** -150         # (a coefficient below fp32's range rounds to 0)
        if what == "loss":
            bound = bound + fp64 * np.abs(np.ones(B) if w is None else w).mean() * np.abs(lw).max()
        err = np.abs(g_ - w_)
        print("K %d B %d %s %s: %.3e (bound %.3e)" % (K, B, objective, what, err.max(), np.max(bound)))
        assert (err <= bound).all(), (what, float(err.max()), float(np.max(bound)))
        assert np.max(bound) <= 1e-4 * np.abs(w_).max() or np.abs(w_).max() == 0
    assert np.isfinite(loss).all() and np.isfinite(c_nll).all()
    if objective == "iwae":
        wb = (np.ones(B) if w is None else w.astype(np.float64)) / B
        assert (np.abs(c_nll.sum(axis=0) - wb) <= K * ((U * SLACK + fp64) * wb + 2.0 ** -150)).all()      # the softmax sums to 1
        assert np.array_equal(c_logpq, -c_nll) and (c_kl == 0).all()
    else:
        assert (c_logpq == 0).all()
    again = F_.bound_objective(dev(parts), dev(logpq), dev(kl), None if w is None else dev(w), objective, beta)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                               # run to run


# ---------------------------------------------------------------------------------------------- ggpm_scale_rows_by_mol
@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("N,ld", [(1, 1), (1, 4), (12, 16), (257, 260)])
@pytest.mark.parametrize("M", [1, 64, 65, 300])
def test_rows_are_scaled_by_their_molecule(M, N, ld, with_g):
    B = 3
    rs = np.random.RandomState(M * 1000 + N)
    d = np.full((M + 2, ld), SENT, np.float32)
    d[:M, :N] = rs.standard_normal((M, N)).astype(np.float32)
    mol = rs.randint(0, B, size=M).astype(np.int32)
    mol[mol == 1] = 0                                   # molecule 1 has no row
    if M >= 64:
        mol[5], mol[17] = -1, B                         # rows of no molecule of this batch
    coef4 = np.full((B, 4), SENT, np.float32)           # a column of dparts [B, 4]: stride 4
    coef4[:, 2] = [0.375, 11.0, -2.7]
    g = np.float32(1.7)
    dd, dc = dev(d), dev(coef4)
    F_.scale_rows_by_mol(dd[:M], N, dev(mol), dc[:, 2], B, dev(np.array([g])) if with_g else None)
    got = f64(dd)
    want = O.scale_rows_by_mol(d[:M], N, mol, coef4[:, 2], B, float(g) if with_g else 1.0)
    err = np.abs(got[:M, :N] - want[:, :N])
    bound = (2 if with_g else 1) * U * SLACK * np.abs(want[:, :N])
    print("M %d N %d ld %d g %d: %.3e (bound %.3e)" % (M, N, ld, with_g, err.max(), bound.max()))
    assert (err <= bound).all()
    assert (got[M:] == SENT).all() and (got[:M, N:] == SENT).all()                          # nothing else is written
    if M >= 64:
        assert (got[5, :N] == 0).all() and (got[17, :N] == 0).all()


# ---------------------------------------------------------------------------------------------- ggpm_latent_terms_backward
def latent_case(K, B, L):
    rs = np.random.RandomState(K * 10000 + B * 100 + L)
    mean = rs.standard_normal((B, L)).astype(np.float32)
    pv = rs.standard_normal((B, L)).astype(np.float32)
    flat = pv.reshape(-1)
    flat[::3] = (rs.standard_normal(len(flat[::3])) * 1e-4).astype(np.float32)
    if flat.size > 2:
        flat[2] = 0.0
    eps = rs.standard_normal((K, B, L)).astype(np.float32)
    dz = rs.standard_normal((K, B, L)).astype(np.float32)
    c_pq = (rs.standard_normal((K, B)) * 0.3).astype(np.float32)
    c_kl = rs.standard_normal(B).astype(np.float32)
    return mean, pv, eps, dz, c_pq, c_kl


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("L", [8, 65])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 3, 65])
def test_latent_backward_equals_fp64_within_the_derived_bounds(K, B, L, with_g):
    mean, pv, eps, dz, c_pq, c_kl = latent_case(K, B, L)
    assert (pv > 0).any() and (pv < 0).any() and (pv == 0).any()
    g = 0.6 if with_g else 1.0
    args = (dev(dz), dev(mean), dev(pv), dev(eps), dev(c_pq), dev(c_kl), dev(np.array([g], np.float32)) if with_g else None)
    dmean, dpv = (f64(t) for t in F_.latent_terms_backward(*args))
    g = float(np.float32(g))
    dm64, dp64 = O.latent_terms_backward(dz, mean, pv, eps, c_pq, c_kl, g)
    m, e = mean.astype(np.float64), eps.astype(np.float64)
    lv = -np.abs(pv.astype(np.float64))
    se = np.abs(np.exp(lv / 2)[None] * e)
    z = m[None] + np.exp(lv / 2)[None] * e
    dz_err = U * (3 * se + np.abs(z))
    G = np.abs(g * c_pq.astype(np.float64))[:, :, None]
    a = np.abs(dz.astype(np.float64) - g * c_pq.astype(np.float64)[:, :, None] * z)
    gk = np.abs(g * c_kl.astype(np.float64))[:, None]
    bm = ((G * dz_err).sum(axis=0) + U * np.abs(dm64)) * SLACK
    dlv = np.abs(dp64)
    bp = ((G * dz_err * se / 2 + a * U * se).sum(axis=0) + gk * U * np.exp(lv) + U * dlv) * SLACK
    em, ep = np.abs(dmean - dm64), np.abs(dpv - dp64)
    print("K %d B %d L %d g %d: dmean %.3e (bound %.3e), dpre_var %.3e (%.3e)" % (K, B, L, with_g, em.max(), bm.max(), ep.max(), bp.max()))
    assert (em <= bm).all(), float((em / bm).max())
    assert (ep <= bp + (pv == 0) * 0).all(), float((ep / np.maximum(bp, 1e-300)).max())
    assert (dpv[pv == 0] == 0).all()                                 # d(-|p|)/dp = 0 at 0, as ggpm_rsample_backward
    assert bm.max() <= 1e-4 * np.abs(dm64).max() and bp.max() <= 1e-4 * np.abs(dp64).max()
    again = F_.latent_terms_backward(*args)
    assert np.array_equal(f64(again[0]), dmean) and np.array_equal(f64(again[1]), dpv)


def test_latent_backward_takes_absent_gradients_as_zeros():
    mean, pv, eps, dz, c_pq, c_kl = latent_case(3, 3, 8)
    for keep in ((True, False, False), (False, True, False), (False, False, True)):
        a = [x if k else None for x, k in zip((dz, c_pq, c_kl), keep)]
        got = F_.latent_terms_backward(None if a[0] is None else dev(a[0]), dev(mean), dev(pv), dev(eps),
                                       None if a[1] is None else dev(a[1]), None if a[2] is None else dev(a[2]))
        z = [np.zeros_like(x) if k is None else k for x, k in zip((dz, c_pq, c_kl), a)]
        full = F_.latent_terms_backward(dev(z[0]), dev(mean), dev(pv), dev(eps), dev(z[1]), dev(z[2]))
        assert all(torch.equal(p, q) for p, q in zip(got, full))


# ---------------------------------------------------------------------------------------------- the attachment head, weighted
UP = 1.5
NAMES = ("rows", "z", "W1", "b1", "Wa", "ba")


@functools.lru_cache(maxsize=None)
def _head(case):
    """Inputs of the existing attachment-head test, its forward state, and the unweighted backward"""
    from motif_fixtures import head_case
    from test_head_kernels_gpu import HEAD_CASES
    H, L, C, B, preds = HEAD_CASES[case]
    inp = head_case(H + L, H, L, C, preds, B, True)
    rows, meta, W1, b1, Wa, ba, z, n_cand = inp
    d = dict(rows=rows.to(DEV), meta=meta.to(DEV), W1=W1.to(DEV), b1=b1.to(DEV), Wa=Wa.to(DEV), ba=ba.to(DEV), z=z.to(DEV))
    Pn = meta.shape[0]
    f32 = dict(dtype=torch.float32, device=DEV)
    d.update(act=torch.empty(rows.shape[0], H, **f32), score=torch.empty(max(n_cand, 1), **f32), stat=torch.empty(Pn, 4, **f32))
    res, counter = torch.empty(2, **f32), torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().ggpm_motif_assm_forward(
        P(d["rows"]), H, P(d["meta"]), Pn, C, H, L, P(d["W1"]), H + 20, P(d["b1"]), P(d["Wa"]), P(d["ba"]), P(d["z"]), L,
        P(d["act"]), P(d["score"]), P(d["stat"]), P(res), P(counter), F_._stream()), "motif_assm_forward")
    return inp, d, (Pn, C, H, L, B)


def _backward(case, coef=None, coef_stride=1, g=UP):
    inp, d, (Pn, C, H, L, B) = _head(case)
    f32 = dict(dtype=torch.float32, device=DEV)
    out = [torch.zeros_like(d["rows"]), torch.zeros_like(d["z"]), torch.empty(H, H + 20, **f32), torch.empty(H, **f32),
           torch.empty_like(d["Wa"]), torch.empty_like(d["ba"])]
    dl = None if g is None else torch.tensor([g], **f32)
    tail = (P(d["rows"]), H, P(d["meta"]), Pn, C, H, L, B, P(d["W1"]), H + 20, P(d["Wa"]), P(d["ba"]), P(d["z"]), L, P(d["act"]),
            P(d["score"]), P(d["stat"]), P(out[0]), P(out[2]), P(out[3]), P(out[4]), P(out[5]), P(out[1]), F_._stream())       # the entry's order: drows, dW1, db1, dWa, dba, dz
    lib = _lib.load()
    if coef is None:
        _lib.check(lib.ggpm_motif_assm_backward(P(dl), *tail), "motif_assm_backward")
    else:
        _lib.check(lib.ggpm_motif_assm_backward_weighted(P(dl), P(coef), coef_stride, *tail), "motif_assm_backward_weighted")
    return out


@pytest.mark.parametrize("case", ["h_P1", "a_W256", "d_H600"])
def test_weighted_attachment_backward(case):
    from motif_fixtures import assm_head_reference
    inp, d, (Pn, C, H, L, B) = _head(case)
    plain = _backward(case)
    # the unweighted entry against fp64 at the existing test's bar: the shared device code still computes what it did
    rows, meta, W1, b1, Wa, ba, z, _ = inp
    rs = np.random.RandomState(H)
    coef = (rs.rand(B) * 3 + 0.2).astype(np.float32)
    coef4 = np.full((B, 4), SENT, np.float32)
    coef4[:, 3] = coef
    for what, c in (("plain", None), ("weighted", coef)):
        ref = [t.double().requires_grad_(True) for t in (rows, z, W1, b1, Wa, ba)]
        total = 0.0
        for b in range(B):
            sub = meta[meta[:, 3] == b]
            if len(sub):
                lb, _ = assm_head_reference(ref[0], sub, C, ref[2], ref[3], ref[4], ref[5], ref[1])
                total = total + (1.0 if c is None else float(c[b])) * lb
        (UP * total).backward()
        got = plain if c is None else _backward(case, dev(coef4)[:, 3], 4)
        for name, a, r in zip(NAMES, got, ref):
            want = r.grad.numpy()
            a = f64(a)
            err = np.abs(a).max() if name == "ba" else np.abs(a - want).max() / max(np.abs(want).max(), 1e-3)
            print("%s %s d%-4s %.2e" % (case, what, name, err))
            assert err <= (1e-5 if name == "ba" else 1e-4), (what, name, err)
    # all-ones weights: g * 1 is exact -> the unweighted entry's output bit for bit; a power of two scales exactly
    ones = _backward(case, torch.ones(B, device=DEV), 1)
    fours = _backward(case, torch.full((B,), 4.0, device=DEV), 1)
    null_g = _backward(case, torch.full((B,), UP, device=DEV), 1, g=None)
    for name, a, b, c4, ng in zip(NAMES, plain, ones, fours, null_g):
        assert torch.equal(a, b), name
        assert torch.equal(a * 4.0, c4), name
        assert torch.equal(a, ng), name
    # a molecule weighted 0 receives no dz and its rows no gradient
    zero = torch.ones(B, device=DEV)
    zero[0] = 0.0
    got = _backward(case, zero, 1)
    assert not bool(got[1][0].ne(0).any())
    m0 = [(int(r), int(n * k)) for n, k, _, b, _, r in inp[1].tolist() if b == 0]
    assert m0 and all(not bool(got[0][r:r + c].ne(0).any()) for r, c in m0)


# ---------------------------------------------------------------------------------------------- the unweighted entry, as before
DIGEST_CASES = ("h_P1", "a_W256", "d_H600", "i_P700")
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol_objective", "assm_backward_digests.json")


def assm_backward_digest(lib, case, distinct):
    """sha256 over the six outputs (drows, dW1, db1, dWa, dba, dz) of ``lib``'s ggpm_motif_assm_backward under an upstream
    factor of 1.5, on the inputs of the existing attachment-head test"""
    import hashlib
    from motif_fixtures import head_case
    from test_head_kernels_gpu import HEAD_CASES
    H, L, C, B, preds = HEAD_CASES[case]
    rows, meta, W1, b1, Wa, ba, z, n_cand = [t.to(DEV) if isinstance(t, torch.Tensor) else t
                                             for t in head_case(H + L, H, L, C, preds, B, distinct)]
    Pn = meta.shape[0]
    f32 = dict(dtype=torch.float32, device=DEV)
    act, score, stat = torch.empty(rows.shape[0], H, **f32), torch.empty(max(n_cand, 1), **f32), torch.empty(Pn, 4, **f32)
    res, counter = torch.empty(2, **f32), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.ggpm_motif_assm_forward(P(rows), H, P(meta), Pn, C, H, L, P(W1), H + 20, P(b1), P(Wa), P(ba), P(z), L, P(act),
                                       P(score), P(stat), P(res), P(counter), None) == 0
    out = [torch.zeros_like(rows), torch.empty(H, H + 20, **f32), torch.empty(H, **f32), torch.empty_like(Wa),
           torch.empty_like(ba), torch.zeros_like(z)]
    dl = torch.tensor([UP], **f32)
    assert lib.ggpm_motif_assm_backward(P(dl), P(rows), H, P(meta), Pn, C, H, L, B, P(W1), H + 20, P(Wa), P(ba), P(z), L, P(act),
                                        P(score), P(stat), *[P(t) for t in out], None) == 0
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in out:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("case", DIGEST_CASES)
def test_unweighted_attachment_backward_is_bit_identical_to_before(case, distinct):
    """the digests were recorded on an MI355X from the library of the commit before the weighted entry was added"""
    import json
    want = json.load(open(DIGESTS))["%s/%d" % (case, distinct)]
    assert assm_backward_digest(_lib.load(), case, distinct) == want


# ---------------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_are_refused_before_any_launch():
    lib, s = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    wk = torch.zeros(8, dtype=torch.float64, device=DEV)
    obj = lambda **kw: lib.ggpm_bound_objective(*[kw.get(k, v) for k, v in (
        ("parts", P(f)), ("logpq", P(f)), ("kl", P(f)), ("w", None), ("K", 2), ("B", 3), ("objective", 0), ("beta", 1.0),
        ("work", P(wk)), ("loss", P(f)), ("c_nll", P(f)), ("c_logpq", P(f)), ("c_kl", P(f)))], s)
    assert obj(K=0) == ERR_ARG and obj(K=1025) == ERR_ARG and obj(B=0) == ERR_ARG
    assert obj(objective=2) == ERR_ARG and obj(objective=1, beta=0.5) == ERR_ARG
    assert obj(work=None) == ERR_ARG and obj(c_kl=None) == ERR_ARG and obj(parts=None) == ERR_ARG
    assert lib.ggpm_scale_rows_by_mol(P(f), 3, 8, 4, P(i), P(f), 1, 3, None, s) == ERR_ARG            # ld < N
    assert lib.ggpm_scale_rows_by_mol(P(f), 4, 8, 4, None, P(f), 1, 3, None, s) == ERR_ARG
    assert lib.ggpm_scale_rows_by_mol(P(f), 4, 8, 4, P(i), P(f), 0, 3, None, s) == ERR_ARG            # stride 0
    assert lib.ggpm_scale_rows_by_mol(P(f), 4, 0, 4, P(i), P(f), 1, 3, None, s) == ERR_ARG
    assert lib.ggpm_scale_rows_by_mol(P(f), 4, 8, 4, P(i), P(f), 1, 0, None, s) == ERR_ARG
    ltb = lib.ggpm_latent_terms_backward
    assert ltb(P(f), P(f), P(f), P(f), P(f), P(f), None, 0, 3, 8, P(f), P(f), s) == ERR_ARG
    assert ltb(P(f), P(f), P(f), P(f), P(f), P(f), None, 1025, 3, 8, P(f), P(f), s) == ERR_ARG
    assert ltb(P(f), P(f), P(f), None, P(f), P(f), None, 2, 3, 8, P(f), P(f), s) == ERR_ARG
    assert ltb(P(f), P(f), P(f), P(f), P(f), P(f), None, 2, 3, 8, None, P(f), s) == ERR_ARG
    w = lib.ggpm_motif_assm_backward_weighted
    rest = (P(f), 8, P(i), 1, 2, 8, 8, 1, P(f), 28, P(f), P(f), P(f), 8, P(f), P(f), P(f), P(f), P(f), P(f), P(f), P(f), P(f), s)
    assert w(None, None, 1, *rest) == ERR_ARG                                                         # no coefficients
    assert w(None, P(f), 0, *rest) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all() and not bool(wk.ne(0).any())                               # nothing ran
