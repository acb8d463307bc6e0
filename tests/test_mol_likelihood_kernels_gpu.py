"""GPU: the kernels behind ``log_likelihood`` called on their own (csrc/mol_loss.hip, the latent draw of csrc/sample.hip)
against the fp64 numpy forms of tests/likelihood_oracle.py, at the smallest shapes that can break them: row counts around
one wave, molecules without rows, an absent term, latent widths and sample counts around 64, log-variances near 0 and
near -30, and log-weights 80 apart.

Bounds, with u = 2^-24 (half an fp32 ulp, relative):
  * parts: exact fp32 inputs, fp64 accumulation, one rounding -> 2u |ref|.
  * z = mean + expf(lv / 2) * eps: expf is within 1 ulp (2u; the HIP math API's stated bound), the product and the sum round
    once each (fewer when contracted) -> u (3 |s eps| + |z|).
  * kl = -0.5 sum_j a_j with the fp32 addend a = ((1 + lv) - m m) - expf(lv) of the training kernel: roundings of 1 + lv, m m,
    their difference and the last difference, and expf's 2u -> 0.5 u sum_j (|1 + lv| + |m m| + |c| + 2 e^lv + |a|), plus the
    final rounding u |kl|.
  * logpq: fp64 arithmetic on the stored z -> sum_j (|z| dz_j + dz_j^2 / 2) + u |logpq|.
  * elbo, iwae: fp64 arithmetic on exact inputs -> one rounding u |ref|, plus what (K + 16) fp64 operations at the scale of the
    largest log-weight can add.
Every bound is also asserted to stay under the project's 1e-4 norm-wise parity figure.  The measured maxima are printed."""
import ctypes

import numpy as np
import pytest
import torch

import likelihood_oracle as LO
import sample_oracle as SO
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT = -777.25
ERR_ARG = 1
P = F_._p
SEED = 0x5EED0123456789AB
SLACK = 1.0 + 2.0 ** -10          # second-order terms of the first-order bounds


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def under_parity(bound, ref):
    assert float(np.max(bound)) <= 1e-4 * float(np.abs(ref).max()), (float(np.max(bound)), float(np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------- ggpm_mol_loss_parts
ROWS = [(1, 63, 64, 65), (257, 65, 1, 63), (64, 257, 0, 1), (65, 1, 257, 0)]


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("rows", ROWS)
def test_parts_equal_the_fp64_sums(B, rows):
    rs = np.random.RandomState(B * 1000 + sum(rows))
    terms_np, terms_dev, keep = [], [], []
    for t, n in enumerate(rows):
        if n == 0:
            terms_np.append(None)
            terms_dev.append(None)          # an absent term: null pointers, 0 rows
            continue
        stride = 4 if t == 3 else 1         # (the tree-only attachment head keeps its losses 4 floats apart)
        v = (rs.rand(n) * 10.0 ** rs.randint(-3, 3, size=n)).astype(np.float32)
        mol = rs.randint(0, B, size=n).astype(np.int32)
        if B > 1:
            mol[mol == 1] = 0               # molecule 1 has no row in any term
        if n >= 63:
            mol[5], mol[17] = -1, B         # rows of no molecule of this batch count nowhere
        buf = np.full(n * stride + 8, SENT, np.float32)
        buf[:n * stride:stride] = v
        dv, dm = dev(buf), dev(np.concatenate([mol, np.full(8, 0, np.int32)]))
        keep += [dv, dm]
        terms_np.append((v, mol))
        terms_dev.append((dv, dm, n, stride))
    out = torch.full((B + 2, 4), SENT, device=DEV)
    got = F_.mol_loss_parts(terms_dev, B, out=out[:B]).cpu().numpy().astype(np.float64)
    assert (out[B:].cpu().numpy() == SENT).all()
    want = LO.mol_parts(terms_np, B)
    err = np.abs(got - want)
    print("B %d rows %s: largest relative distance %.3e" % (B, rows, float((err / np.maximum(want, 1e-300)).max())))
    assert (err <= 2 * U * np.abs(want)).all()
    if B > 1:
        assert (got[1] == 0).all()
    for t, n in enumerate(rows):
        if n == 0:
            assert (got[:, t] == 0).all()
    again = F_.mol_loss_parts(terms_dev, B).cpu().numpy()
    assert np.array_equal(again, got.astype(np.float32))           # run to run


# ---------------------------------------------------------------------------------------------- ggpm_latent_terms
SHAPES = [(1, 1, 1), (2, 3, 8), (5, 65, 24), (65, 3, 65), (1, 65, 65), (2, 1, 24)]


def latent_case(K, B, L):
    rs = np.random.RandomState(K * 10000 + B * 100 + L)
    mean = rs.standard_normal((B, L)).astype(np.float32)
    pv = rs.standard_normal((B, L)).astype(np.float32)
    flat = pv.reshape(-1)
    flat[::3] = (rs.standard_normal(len(flat[::3])) * 1e-4).astype(np.float32)             # lv near 0
    flat[1::5] = (30.0 + rs.standard_normal(len(flat[1::5])) * 0.1).astype(np.float32) * rs.choice([-1, 1], len(flat[1::5]))
    if flat.size > 2:
        flat[2] = 0.0
    eps = rs.standard_normal((K, B, L)).astype(np.float32)
    return mean, pv, eps


@pytest.mark.parametrize("K,B,L", SHAPES)
def test_latent_terms_equal_fp64_within_the_derived_bounds(K, B, L):
    mean, pv, eps = latent_case(K, B, L)
    z, kl, logpq = (t.cpu().numpy().astype(np.float64) for t in F_.latent_terms(dev(mean), dev(pv), dev(eps)))
    z64, kl64, pq64 = LO.latent_terms(mean, pv, eps)
    m, e = mean.astype(np.float64), eps.astype(np.float64)
    lv = -np.abs(pv.astype(np.float64))
    se = np.exp(lv / 2)[None] * e
    dz = U * (3 * np.abs(se) + np.abs(z64)) * SLACK
    assert (np.abs(z - z64) <= dz).all(), float((np.abs(z - z64) / dz).max())
    a1, mm, ex = 1 + lv, m * m, np.exp(lv)
    c = a1 - mm
    dkl = (0.5 * U * (np.abs(a1) + mm + np.abs(c) + 2 * ex + np.abs(c - ex)).sum(axis=1) + U * np.abs(kl64)) * SLACK
    assert (np.abs(kl - kl64) <= dkl).all(), float((np.abs(kl - kl64) / dkl).max())
    dpq = ((np.abs(z64) * dz + 0.5 * dz * dz).sum(axis=2) + U * np.abs(pq64)) * SLACK
    assert (np.abs(logpq - pq64) <= dpq).all(), float((np.abs(logpq - pq64) / dpq).max())
    print("K %d B %d L %d: z %.3e (bound %.3e), kl %.3e (%.3e), logpq %.3e (%.3e)" % (
        K, B, L, np.abs(z - z64).max(), dz.max(), np.abs(kl - kl64).max(), dkl.max(), np.abs(logpq - pq64).max(), dpq.max()))
    if B * L >= 24:                        # (a single element can be arbitrarily close to 0: the figure is norm-wise)
        under_parity(dz, z64), under_parity(dkl, kl64), under_parity(dpq, pq64)


def test_latent_terms_zero_eps_is_the_mean_and_logpq_the_entropy_term():
    mean, pv, _ = latent_case(1, 65, 24)
    z, kl, logpq = F_.latent_terms(dev(mean), dev(pv), torch.zeros(1, 65, 24, device=DEV))
    assert np.array_equal(z[0].cpu().numpy(), mean)
    again = F_.latent_terms(dev(mean), dev(pv), torch.zeros(1, 65, 24, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip((z, kl, logpq), again))


# ---------------------------------------------------------------------------------------------- ggpm_iwae_finish
@pytest.mark.parametrize("K", [1, 2, 5, 65])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_finish_equals_fp64_with_log_weights_80_apart(K, B):
    rs = np.random.RandomState(K * 100 + B)
    parts = (rs.rand(K, B, 4) * 2).astype(np.float32)
    if K > 1:
        parts[:, :, 0] += np.linspace(20.0, 100.0, K).astype(np.float32)[rs.permutation(K)][:, None]     # nll spread 80 over k
    parts[:, B // 2, 3] = 0.0                                     # a molecule without attachment predictions
    logpq = (rs.standard_normal((K, B)) * 3).astype(np.float32)
    logpq[:, 0] += 200.0                                          # exp() of these log-weights overflows fp32
    kl = (rs.rand(B) * 4).astype(np.float32)
    elbo, iwae = (t.cpu().numpy().astype(np.float64) for t in F_.iwae_finish(dev(parts), dev(logpq), dev(kl)))
    elbo64, iwae64 = LO.iwae_finish(parts, logpq, kl)
    nll = parts.astype(np.float64).sum(axis=2)
    w = logpq.astype(np.float64) - nll
    if K > 1:
        assert (w.max(axis=0) - w.min(axis=0)).min() > 60 and np.abs(w).max() > 88           # past fp32's exp range both ways
    fp64_ops = (K + 16) * 2.0 ** -52 * max(np.abs(w).max(), nll.max())
    for got, want, what in ((elbo, elbo64, "elbo"), (iwae, iwae64, "iwae")):
        bound = U * np.abs(want) * SLACK + fp64_ops
        err = np.abs(got - want)
        print("K %d B %d %s: %.3e (bound %.3e)" % (K, B, what, err.max(), bound.max()))
        assert (err <= bound).all(), (what, float((err / bound).max()))
        under_parity(bound, want)
    if K == 1:                              # the single-sample ELBO estimate
        assert np.abs(iwae - (logpq[0].astype(np.float64) - nll[0])).max() <= (U * np.abs(iwae64) * SLACK + fp64_ops).max()
    assert np.isfinite(iwae).all() and np.isfinite(elbo).all()


# ---------------------------------------------------------------------------------------------- the latent draw
def draw(K, B, L, ids, seed=SEED):
    lo, hi = SO.split(seed)
    out = torch.full((K * B * L + 8,), SENT, device=DEV)
    keep = dev((np.asarray(ids, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    assert _lib.load().ggpm_sample_latent_normal(P(out), K, B, L, P(keep), lo, hi, F_._stream()) == 0
    out = out.cpu().numpy()
    assert (out[K * B * L:] == SENT).all()
    return out[:K * B * L].reshape(K, B, L)


@pytest.mark.parametrize("K,B,L", [(2, 3, 8), (5, 65, 24), (65, 3, 65), (65, 7, 1)])
def test_latent_normals_equal_the_restatement(K, B, L):
    """under 4 times the distance of numpy's own fp32 evaluation from fp64, as the prior's normals are"""
    ids = (np.random.RandomState(B).choice(1 << 22, size=B, replace=False).astype(np.int64) * 1021 + 17)
    ids[::5] += 1 << 31
    want = LO.latent_normals(SEED, ids, K, L)
    bound = 4.0 * float(np.abs(LO.latent_normals(SEED, ids, K, L, np.float32).astype(np.float64) - want).max())
    got = draw(K, B, L, ids)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("K %d B %d L %d: distance %.3e, bound %.3e" % (K, B, L, err, bound))
    assert err <= bound


def test_latent_normals_prefix_batch_independence_and_site():
    ids = np.array([5, 900, 33, (1 << 31) + 2, 77])
    full = draw(65, 5, 24, ids)
    assert np.array_equal(draw(3, 5, 24, ids), full[:3])                          # the first K draws of a larger call
    perm = np.array([3, 0, 4, 1, 2])
    assert np.array_equal(draw(65, 5, 24, ids[perm]), full[:, perm])              # a molecule's draws follow its id
    assert np.array_equal(draw(65, 1, 24, ids[[2]]), full[:, [2]])                # ... not the batch size
    assert not np.array_equal(draw(3, 5, 24, ids, SEED + 1), full[:3])
    lo, hi = SO.split(SEED)
    got = F_.sample_latent_normal(3, 5, 24, lo, hi, ids=ids, device=DEV).cpu().numpy()
    assert np.array_equal(got, full[:3])
    # the prior's stream is another site: same ids, same counters (k = 0), other values
    prior = F_.sample_normal(5, 24, lo, hi, ids=ids, device=DEV).cpu().numpy()
    assert not np.array_equal(prior, full[0])
    z = draw(16, 512, 32, np.arange(512)).astype(np.float64).reshape(-1)
    assert abs(z.mean()) <= 5 / np.sqrt(z.size) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / z.size)


def test_bad_arguments_are_refused_before_any_launch():
    lib, s = _lib.load(), F_._stream()
    f = torch.full((4096,), SENT, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    terms = (F_.MolLossTerm * 4)()
    terms[0] = F_.MolLossTerm(f.data_ptr(), i.data_ptr(), 0, 8)                   # stride 0
    assert lib.ggpm_mol_loss_parts(ctypes.byref(terms), 3, P(f), s) == ERR_ARG
    terms[0] = F_.MolLossTerm(f.data_ptr(), None, 1, 8)                           # rows without their molecules
    assert lib.ggpm_mol_loss_parts(ctypes.byref(terms), 3, P(f), s) == ERR_ARG
    terms[0] = F_.MolLossTerm(f.data_ptr(), i.data_ptr(), 1, 8)
    assert lib.ggpm_mol_loss_parts(ctypes.byref(terms), 0, P(f), s) == ERR_ARG
    assert lib.ggpm_latent_terms(P(f), P(f), P(f), 1025, 1, 2, P(f), P(f), P(f), s) == ERR_ARG
    assert lib.ggpm_latent_terms(P(f), P(f), P(f), 2, 3, 0, P(f), P(f), P(f), s) == ERR_ARG
    assert lib.ggpm_latent_terms(P(f), P(f), None, 2, 3, 8, P(f), P(f), P(f), s) == ERR_ARG
    assert lib.ggpm_iwae_finish(P(f), P(f), P(f), 0, 3, P(f), P(f), s) == ERR_ARG
    assert lib.ggpm_iwae_finish(P(f), P(f), P(f), 2, 3, None, P(f), s) == ERR_ARG
    assert lib.ggpm_sample_latent_normal(P(f), 0, 3, 8, P(i), 1, 2, s) == ERR_ARG
    assert lib.ggpm_sample_latent_normal(P(f), 2, 3, 8, None, 1, 2, s) == ERR_ARG
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == SENT).all()                                         # nothing ran
