"""The seeded stream of the sampled decode and of the prior, restated in numpy from DESIGN.md (*Sampled decoding and the
prior*): the 24-bit words in 32-bit integer arithmetic, the three draws in fp64 (``dtype=np.float32`` runs the same
expressions in fp32, which is how the tests size what an fp32 evaluation may differ by), and a host ``sampler`` for the
decode loop's ``sampler=`` seam built on them.  CPU only."""
import numpy as np

SITE_TOPO, SITE_BEAM, SITE_PRIOR = 256, 257, 258        # include/ggpm_hip.h GGPM_SITE_SAMPLE_*
MAX_K = 16
MARGIN = 1e-4       # the project's decision margin (tests/golden/make_golden_decode.py)
_M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, np.uint64) & _M32


def fmix32(h):
    """the murmur3 32-bit finaliser, on uint64 arrays holding 32-bit values"""
    h = _u(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def split(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def words(seed, site, ids, step, slot):
    """m(site, id, step, slot), broadcast over ids / step / slot -> uint64 array of 24-bit values"""
    lo, hi = split(seed)
    ids, step, slot = _u(np.asarray(ids, np.int64)), _u(step), _u(slot)
    base = fmix32(fmix32((ids * np.uint64(0x9E3779B1) + np.uint64(lo)) & _M32)
                  ^ ((np.uint64(hi) + np.uint64(site) * np.uint64(0x7F4A7C15)) & _M32))
    ctr = (((step * np.uint64(64)) & _M32) + slot) & _M32
    return fmix32((base + ((ctr * np.uint64(0x9E3779B1)) & _M32)) & _M32) >> np.uint64(8)


def topo_uniforms(seed, ids, step):
    return words(seed, SITE_TOPO, ids, step, 0).astype(np.float64) * 2.0 ** -24


def topo_draws(seed, ids, step, p):
    """draw = m 2^-24 < p (exact in fp32 as in fp64) -> float 0.0 / 1.0"""
    return (topo_uniforms(seed, ids, step) < np.asarray(p, np.float64)).astype(np.float64)


def beam_keys(seed, ids, step, scores, dtype=np.float64):
    """key_q = score_q - log(e_q), e_q = max(-log((m_q + 1) 2^-24), 2^-24) -> [M, k]"""
    scores = np.asarray(scores, dtype)
    M, k = scores.shape
    m = words(seed, SITE_BEAM, np.asarray(ids).reshape(M, 1), step, np.arange(k).reshape(1, k))
    u = ((m + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    e = np.maximum(-np.log(u), dtype(2.0 ** -24)).astype(dtype)
    return (scores - np.log(e)).astype(dtype)


def order_of(keys):
    """descending keys, ties to the lower index -> (order [M, k], smallest adjacent key gap per row [M], inf for k = 1)"""
    keys = np.asarray(keys)
    order = np.argsort(-keys, axis=1, kind="stable")
    ranked = np.take_along_axis(keys.astype(np.float64), order, axis=1)
    gaps = -np.diff(ranked, axis=1)
    return order, (gaps.min(axis=1) if keys.shape[1] > 1 else np.full(len(keys), np.inf))


def beam_order(seed, ids, step, scores, dtype=np.float64):
    return order_of(beam_keys(seed, ids, step, scores, dtype))


def normals(seed, ids, cols, dtype=np.float64):
    """Box-Muller: sqrt(-2 log((m0 + 1) 2^-24)) cos(2 pi m1 2^-24), m0 / m1 = m(PRIOR, id, column, 0 / 1) -> [rows, cols]"""
    ids = np.asarray(ids).reshape(-1, 1)
    c = np.arange(cols).reshape(1, -1)
    m0, m1 = words(seed, SITE_PRIOR, ids, c, 0), words(seed, SITE_PRIOR, ids, c, 1)
    u1 = ((m0 + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    u2 = (m1.astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u1)).astype(dtype)
    return (r * np.cos(dtype(np.pi) * (dtype(2.0) * u2))).astype(dtype)


class Sampler:
    """the decode loop's ``sampler=`` on the restated stream.  ``order`` ranks by the scores, as the device does (the
    probabilities of masked entries are all 0 and would not tell them apart); ``n_masked_rows`` counts the rows it met with
    two or more masked entries.  Keeps the smallest distance of a topology probability from
    its uniform (``topo_margin``) and the smallest adjacent key gap (``order_margin``) it met: a device decode can be asked
    to agree with this one only when both stay above what fp32 resolves."""

    def __init__(self, seed):
        self.seed = seed
        self.topo_margin = self.order_margin = np.inf
        self.n_topo = self.n_order = self.n_masked_rows = 0

    def topo(self, step, mol_ids, probs):
        u = topo_uniforms(self.seed, mol_ids, step)
        self.topo_margin = min(self.topo_margin, float(np.abs(u - probs).min()))
        self.n_topo += len(u)
        return topo_draws(self.seed, mol_ids, step, probs)

    def order(self, step, mol_ids, probs, scores):
        scores = np.asarray(scores, np.float64)
        assert np.all(np.abs(np.exp(scores) - probs) <= 1e-12)
        self.n_masked_rows += int(((scores < -500).sum(axis=1) >= 2).sum())
        order, gaps = beam_order(self.seed, mol_ids, step, scores)
        assert not np.isnan(gaps).any()
        self.order_margin = min(self.order_margin, float(gaps.min()))
        self.n_order += len(order)
        return order


class Replay:
    """the decode loop's ``sampler=`` returning recorded draws in order: ``topo`` / ``order`` are lists of (input, output)
    as the reference's ``torch.bernoulli`` / ``torch.multinomial`` calls saw them.  Every call's input must equal the
    recorded one within ``tol``."""

    def __init__(self, topo, order, tol):
        self.topo_calls, self.order_calls, self.tol = list(topo), list(order), tol
        self.i_topo = self.i_order = 0

    def _next(self, calls, i, got, what):
        assert i < len(calls), "more %s draws than the reference made" % what
        want, out = calls[i]
        want, got = np.asarray(want, np.float64), np.asarray(got, np.float64)
        assert got.shape == want.shape, (what, i, got.shape, want.shape)
        assert np.all(np.abs(got - want) <= self.tol * np.maximum(1.0, np.abs(want))), (what, i, got, want)
        return np.asarray(out)

    def topo(self, step, mol_ids, probs):
        self.i_topo += 1
        return self._next(self.topo_calls, self.i_topo - 1, probs, "topology")

    def order(self, step, mol_ids, probs, scores):
        self.i_order += 1
        return self._next(self.order_calls, self.i_order - 1, probs, "beam")

    def exhausted(self):
        return self.i_topo == len(self.topo_calls) and self.i_order == len(self.order_calls)
