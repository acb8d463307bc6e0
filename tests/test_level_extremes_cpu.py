"""CPU: the saturating level inputs of tests/level_extreme_cases.py stay saturating, and the oracle stays a reference there.

Conditions of tests/test_gpu_level_extremes.py, checked with the fp64 oracle alone: at least 30 % of the gather-sigmoid
arguments lie beyond 17 and at least 1 % beyond the clamp at 88 (so a change of seeds, of seeded_state_dict or of
random_level cannot move the GPU test back into the unsaturated range unnoticed), and the oracle's own fp32 run is
within 1.5e-5 of its fp64 run on every tensor, a sixfold margin under the 1e-4 bar the kernels are held to."""
import numpy as np
import pytest
import torch

import level_extreme_cases as X
from golden_utils import rel_err


@pytest.mark.parametrize("shape", X.SHAPES, ids=X.shape_id)
@pytest.mark.parametrize("cell", X.CELLS)
def test_saturating_inputs_saturate_and_the_oracle_holds(cell, shape):
    E, _, H, depth = shape
    sd, x, bgraph, w = X.saturating(cell, E, H)
    a = np.abs(X.gather_sigmoid_arguments(cell, sd, x, bgraph, depth))
    n_pairs = int((bgraph > 0).sum())
    assert a.size == n_pairs * H * (depth - 1)
    beyond17, beyond88 = float((a > 17.0).mean()), float((a > 88.0).mean())
    r64, r32 = (X.oracle_dense(cell, sd, x, bgraph, w, depth, dt) for dt in (torch.float64, torch.float32))
    dist = {k: rel_err(r32[k], r64[k]) for k in r64}
    worst = max(dist, key=dist.get)
    print("saturating %s %s: gather-sigmoid arguments beyond 17: %.1f %%, beyond 88: %.1f %%, largest %.0f; "
          "oracle fp32 - fp64 %.2e (%s)" % (cell, X.shape_id(shape), 100 * beyond17, 100 * beyond88, a.max(), dist[worst], worst))
    assert beyond17 >= 0.30
    assert beyond88 >= 0.01
    assert all(np.isfinite(v).all() for v in r64.values())
    assert (r64["h"][0] == 0).all()
    for k, d in dist.items():
        assert d <= 1.5e-5, (k, d)


def _brute_force_masks(cell, sd, x, bgraph, depth):
    """the recurrence in numpy fp64 over real predecessor lists only, NaN and all -> isnan(h), isnan(c)"""
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    P = {k: v.astype(np.float64) for k, v in sd.items()}
    E1, H = x.shape[0], P["U_r.weight" if cell == "GRU" else "W_i.0.weight"].shape[0]
    x = x.astype(np.float64)
    h, c = np.zeros((E1, H)), np.zeros((E1, H))
    lists = [row[row > 0] for row in bgraph]
    with np.errstate(all="ignore"):
        for d in range(depth):
            hn, cn = np.zeros_like(h), np.zeros_like(c)
            for e in range(1, E1):
                hp, cp = h[lists[e]], c[lists[e]]
                s = hp.sum(axis=0)
                live = d > 0 and len(lists[e]) > 0        # (what the kernels evaluate: no list at h = 0, none when empty)
                if cell == "GRU":
                    g = np.zeros(H)
                    if live:
                        r = sig(P["W_r.weight"] @ x[e] + hp @ P["U_r.weight"].T + P["U_r.bias"])
                        g = (r * hp).sum(axis=0)
                    z = sig(P["W_z.weight"] @ np.concatenate([x[e], s]) + P["W_z.bias"])
                    m = np.tanh(P["W_h.weight"] @ np.concatenate([x[e], g]) + P["W_h.bias"])
                    hn[e] = (1 - z) * s + z * m
                else:
                    xs = np.concatenate([x[e], s])
                    fc = np.zeros(H)
                    if live:
                        Wf = P["W_f.0.weight"]
                        f = sig(Wf[:, :X.I] @ x[e] + P["W_f.0.bias"] + hp @ Wf[:, X.I:].T)
                        fc = (f * cp).sum(axis=0)
                    i, o = (sig(P[n + ".weight"] @ xs + P[n + ".bias"]) for n in ("W_i.0", "W_o.0"))
                    cn[e] = i * np.tanh(P["W.0.weight"] @ xs + P["W.0.bias"]) + fc
                    hn[e] = o * np.tanh(cn[e])
            h, c = hn, cn
    return np.isnan(h), np.isnan(c)


@pytest.mark.parametrize("depth", X.POISON_DEPTHS)
@pytest.mark.parametrize("poison", X.POISON, ids=X.poison_id)
def test_poison_masks_follow_the_recurrence_over_real_lists(poison, depth):
    """poison_nan_masks (what the GPU test expects) against the recurrence written out in numpy, on the small shape: the
    NaN pattern of rows with predecessors, and nothing else touched.  (The padded oracle cannot serve: its h * mask and its
    pad slots compute NaN * 0.)"""
    cell, name, half = poison
    E, _, H, _ = X.SHAPES[0]
    sd, x, bgraph, _ = X.clean(cell, E, H)
    j, index = X.poison_element(cell, name, half, H)
    nh, nc = X.poison_nan_masks(cell, bgraph, H, depth, j)
    bh, bc = _brute_force_masks(cell, X.poisoned(sd, name, index), x, bgraph, depth)
    assert np.array_equal(nh, bh) and np.array_equal(nc, bc)
    has = (bgraph > 0).any(axis=1)
    assert 0 < has.sum() < E and not nh[~has].any() and nh[has][:, j].all()
    if cell == "GRU":
        assert nh[has].all()
    elif depth == 2:
        assert nh.sum() == has.sum()           # column j alone
    else:                                        # whole rows wherever a predecessor had predecessors; column j otherwise
        full = nh.all(axis=1)
        assert full.any() and (nh[has & ~full].sum(axis=1) == 1).all()
