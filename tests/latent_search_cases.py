"""The shapes the guided latent search is checked at (tests/test_latent_search_kernels_gpu.py), built without a GPU so that
tests/test_latent_search_oracle_cpu.py can hold every one of them to its conditions first: in the oracle's fp64 run every
decision keeps a relative margin of at least 1e-4, and the fp32 run takes the same decisions.

Heads: W ~ N(0, (gain / sqrt(fan-in))^2) and hidden biases of magnitude 0.5 .. 1 with random signs (unit 0 positive), so that
a unit is clearly on or clearly off and few cross their kink during a short trajectory; a wide layer of generic weights has
thousands of units per evaluation and one of them always lands within 1e-4 of zero."""
import functools

import numpy as np

import latent_search_oracle as lso

MIN_MARGIN = 1e-4


def make_head(rs, widths, gain):
    layers = []
    for i in range(len(widths) - 1):
        win, wout = widths[i], widths[i + 1]
        if i < len(widths) - 2:
            W = rs.standard_normal((wout, win)) * (gain / np.sqrt(win))
            b = rs.choice([-1.0, 1.0], wout) * rs.uniform(0.5, 1.0, wout)
            b[0] = abs(b[0])
        else:
            W = rs.standard_normal((wout, win)) * (2.0 / np.sqrt(win))
            b = rs.standard_normal(wout) * 0.3
        layers.append((W.astype(np.float32), b.astype(np.float32)))
    return layers


def make_prior(rs, C, L):
    """(logits [C], means [C, L], log_vars [C, L]) fp32, or None for C = 0"""
    if C == 0:
        return None
    return (rs.standard_normal(C).astype(np.float32), (0.7 * rs.standard_normal((C, L))).astype(np.float32),
            (0.3 * rs.standard_normal((C, L))).astype(np.float32))


# name: half, hidden widths of the homo / lumo head, B, K, columns past L, C (0: standard normal), steps, delta, momentum,
#       anchor_weight, prior_weight, lr, (w_h, w_l), gain, seed
CASES = {
    # the smallest of everything: one lane at work in each half, one component, pass-through columns
    "half1_width1": (1, [1], [1], 1, 1, 3, 1, 25, -1.0, 0.0, 0.3, 0.2, 0.05, (1.0, 1.0), 0.25, 11),
    # the configuration's shape, all three terms under the standard normal, three starts of five molecules
    "half12_normal": (12, [65], [65], 5, 3, 0, 0, 25, -1.0, 0.9, 0.02, 0.02, 0.02, (1.0, 0.5), 0.25, 22),
    # heads of different depth (2 and 4 Linear layers), half past one wave, five components
    "half70_depths": (70, [65], [65, 33, 17], 5, 3, 5, 5, 20, -1.0, 0.9, 0.4, 0.2, 0.02, (1.0, 1.0), 0.25, 13),
    # half past 128 lanes (a second trip of every lane loop), more than 64 KiB of LDS, components past two waves' stride
    "half130_c130": (130, [65], [65], 1, 3, 1, 130, 12, -1.0, 0.9, 0.3, 0.3, 0.02, (1.0, 1.0), 0.25, 14),
    # the widest hidden layer with the weights resident; plain descent on prop alone (both weights 0, no momentum)
    "width512_plain": (12, [512], [512], 5, 1, 0, 0, 15, -1.0, 0.0, 0.0, 0.0, 0.05, (1.0, 1.0), 0.15, 24),
    # three hidden layers of 512: the weights do not fit beside the rest and are read from global memory
    "global_weights": (12, [512, 512, 512], [512, 512, 512], 1, 1, 0, 5, 3, -1.0, 0.9, 0.3, 0.2, 0.2, (1.0, 1.0), 0.5, 20),
    # the delta exit: at step 0 for every row / mid-run for most rows and never for three; one molecule's best start is not 0
    "delta_at_0": (12, [65], [65], 5, 3, 2, 0, 25, 1.0e3, 0.9, 0.5, 0.1, 0.02, (1.0, 1.0), 0.25, 17),
    "delta_mid": (12, [65], [65], 5, 3, 2, 1, 25, 0.5, 0.9, 0.05, 0.02, 0.03, (1.0, 1.0), 0.25, 25),
}
ORDER = list(CASES)


def inputs(name):
    """-> dict(homo, lumo, z0 [K B, ld], mu, lv [B, L], t_h, t_l [B], prior) of fp32 arrays"""
    half, hid_h, hid_l, B, K, extra, C, _steps, _delta, _mom, _aw, _pw, _lr, _w, gain, seed = CASES[name]
    rs = np.random.RandomState(seed)
    L = 2 * half
    homo, lumo = make_head(rs, [half] + hid_h + [1], gain), make_head(rs, [half] + hid_l + [1], gain)
    mu = (0.8 * rs.standard_normal((B, L))).astype(np.float32)
    lv = (-np.abs(rs.standard_normal((B, L)))).astype(np.float32)
    z0 = np.empty((K, B, L + extra), np.float32)
    z0[:, :, :L] = mu[None] + np.exp(0.5 * lv)[None] * rs.standard_normal((K, B, L))
    z0[0, :, :L] = mu
    z0[:, :, L:] = rs.standard_normal((K, B, extra))
    return dict(homo=homo, lumo=lumo, z0=z0.reshape(K * B, L + extra), mu=mu, lv=lv,
                t_h=rs.standard_normal(B).astype(np.float32), t_l=rs.standard_normal(B).astype(np.float32),
                prior=make_prior(rs, C, L))


def run(name, dtype, margins=None, inp=None, rows=None):
    """the oracle on case ``name`` (``rows``: only molecule ``rows`` of it, as a batch of one)"""
    half, _, _, B, K, _extra, _C, steps, delta, mom, aw, pw, lr, (w_h, w_l), _, _ = CASES[name]
    x = inp or inputs(name)
    z0, mu, lv, t_h, t_l = x["z0"], x["mu"], x["lv"], x["t_h"], x["t_l"]
    if rows is not None:
        z0 = z0.reshape(K, B, -1)[:, rows:rows + 1].reshape(K, -1)
        mu, lv, t_h, t_l, B = mu[rows:rows + 1], lv[rows:rows + 1], t_h[rows:rows + 1], t_l[rows:rows + 1], 1
    return lso.search(x["homo"], x["lumo"], z0, half, mu, lv, t_h, t_l, K, B, lr, mom, steps, delta, w_h, w_l, aw, pw,
                      prior=x["prior"], dtype=dtype, margins=margins)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (inputs, fp32 run, fp64 run, fp32 margins, fp64 margins); computed once, shared, not to be written to"""
    x = inputs(name)
    m32, m64 = lso.Margins(), lso.Margins()
    return x, run(name, np.float32, m32, x), run(name, np.float64, m64, x), m32, m64


def bounds(r32, r64):
    """per element max(1e-4, 4 |oracle fp32 - oracle fp64|) for z, pred, terms and J"""
    return {k: np.maximum(1e-4, 4 * np.abs(r32[k].astype(np.float64) - r64[k])) for k in ("z", "pred", "terms", "J")}
