"""CPU: the restatement of the guided latent search (tests/latent_search_oracle.py) against what it must be by itself -- its
gradient against finite differences of its own objective, plain descent by hand on a one-unit head, descent that descends, the
selection rule -- and the conditions every GPU case (tests/latent_search_cases.py) must meet before a device result is
compared with it."""
import os
import re

import numpy as np
import pytest

import latent_search_cases as lc
import latent_search_oracle as lso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed, half, hidden, C):
    rs = np.random.RandomState(seed)
    L = 2 * half
    homo, lumo = lc.make_head(rs, [half] + hidden + [1], 0.6), lc.make_head(rs, [half] + hidden + [1], 0.6)
    mu, lv = 0.5 * rs.standard_normal(L), -np.abs(rs.standard_normal(L))
    return homo, lumo, rs.standard_normal(L), mu, lv, 0.3, -0.7, lc.make_prior(rs, C, L)


@pytest.mark.parametrize("C", [0, 5])
def test_gradient_matches_central_differences_of_the_objective(C):
    """all three terms at once; C = 0 is the standard normal.  (The units' margins are checked first: a difference quotient
    across a ReLU kink measures nothing.)"""
    half = 6
    homo, lumo, v, mu, lv, th, tl, prior = _problem(3 + C, half, [9, 7], C)
    args = (half, mu, lv, th, tl, 1.3, 0.6, 0.7, 0.4, prior)
    m = lso.Margins()
    heads = (lso._cast(homo, np.float64), lso._cast(lumo, np.float64))
    lso._heads(heads, v, half, m)
    assert m.min > 1e-3
    J, g = lso.objective(homo, lumo, v, *args)
    h = 1e-6
    for j in range(2 * half):
        e = np.zeros(2 * half)
        e[j] = h
        fd = (lso.objective(homo, lumo, v + e, *args)[0] - lso.objective(homo, lumo, v - e, *args)[0]) / (2 * h)
        assert abs(fd - g[j]) <= 1e-6 * max(1.0, abs(g[j])), (j, fd, g[j])


def test_each_term_alone_has_its_textbook_gradient():
    half = 4
    homo, lumo, v, mu, lv, th, tl, prior = _problem(9, half, [5], 3)
    _, g_anchor = lso.objective(homo, lumo, v, half, mu, lv, th, tl, 0.0, 0.0, 1.0, 0.0)
    assert np.allclose(g_anchor, (v - mu) * np.exp(-lv), rtol=1e-12, atol=0)
    _, g_normal = lso.objective(homo, lumo, v, half, mu, lv, th, tl, 0.0, 0.0, 0.0, 1.0)
    assert np.allclose(g_normal, v, rtol=1e-12, atol=0)
    one = (np.zeros(1, np.float32), np.zeros((1, 2 * half), np.float32), np.zeros((1, 2 * half), np.float32))
    J_mix, g_mix = lso.objective(homo, lumo, v, half, mu, lv, th, tl, 0.0, 0.0, 0.0, 1.0, prior=one)
    J_n, _ = lso.objective(homo, lumo, v, half, mu, lv, th, tl, 0.0, 0.0, 0.0, 1.0)
    assert abs(J_mix - J_n) <= 1e-12 * abs(J_n) and np.allclose(g_mix, v, rtol=1e-12, atol=1e-15)


def test_plain_descent_on_a_one_unit_head_by_hand():
    """both weights 0, momentum 0, K = 1: v <- v - lr 2 (o - t) w2 w1 while the unit is on, with o = w2 relu(w1 v + b1) + b2"""
    w1, b1, w2, b2 = 0.5, 0.25, -1.5, 0.125
    head = [(np.array([[w1]]), np.array([b1])), (np.array([[w2]]), np.array([b2]))]
    off = [(np.array([[1.0]]), np.array([-100.0])), (np.array([[1.0]]), np.array([0.0]))]      # never on: no gradient
    v, t, lr = 1.0, 0.5, 0.1
    out = lso.search(head, off, np.array([[v, 3.0]]), 1, np.zeros((1, 2)), np.zeros((1, 2)), [t], [0.0], 1, 1, lr, 0.0, 4, -1.0)
    for _ in range(4):
        o = w2 * max(w1 * v + b1, 0.0) + b2
        v = v - lr * (2.0 * (o - t) * w2 * w1)
    assert out["z"][0, 0] == pytest.approx(v, rel=1e-14)
    assert out["z"][0, 1] == 3.0 and out["steps"][0] == 4 and out["best"][0] == 0
    o = w2 * max(w1 * v + b1, 0.0) + b2
    assert out["pred"][0, 0] == pytest.approx(o, rel=1e-14) and out["pred"][1, 0] == 0.0
    assert out["terms"][0, 0] == pytest.approx((o - t) ** 2, rel=1e-13)
    assert out["J"][0] == out["terms"][0, 0]


def test_objective_does_not_increase_over_a_short_run_with_a_small_step():
    half = 6
    homo, lumo, v, mu, lv, th, tl, prior = _problem(21, half, [9], 4)
    trace = []
    out = lso.search(homo, lumo, v[None], half, mu[None], lv[None], [th], [tl], 1, 1, 1e-3, 0.0, 30, -1.0, 1.0, 1.0, 0.5, 0.3,
                     prior=prior, trace=trace)
    trace.append(float(out["J"][0]))
    assert len(trace) == 31 and all(b <= a for a, b in zip(trace, trace[1:])) and trace[-1] < trace[0]


def test_selection_rule_ties_nan_and_all_nan():
    nan, inf = np.nan, np.inf
    J = np.array([[2.0, 1.0, nan, nan, inf, -inf, 5.0],
                  [1.0, 1.0, 3.0, nan, nan, nan, 5.0],
                  [1.0, 0.5, 2.0, nan, -1.0, 7.0, 4.0]])
    assert lso.select(J.reshape(-1), 3, 7).tolist() == [1, 2, 2, 0, 2, 0, 2]
    assert lso.select(np.array([nan, 1.0]), 1, 2).tolist() == [0, 0]


def test_a_positive_anchor_weight_keeps_the_selected_latent_nearer_its_posterior():
    """what tests/test_latent_search_gpu.py asserts on the fixture model, shown here on the oracle alone: the selected
    latent's anchor term is smaller with anchor_weight > 0 than with 0"""
    name = "half12_normal"
    half, _, _, B, K, _, _, steps, delta, mom, _, pw, lr, (w_h, w_l), _, _ = lc.CASES[name]
    x = lc.inputs(name)
    runs = [lso.search(x["homo"], x["lumo"], x["z0"], half, x["mu"], x["lv"], x["t_h"], x["t_l"], K, B, lr, mom, steps, delta,
                       w_h, w_l, aw, pw) for aw in (0.0, 0.5)]
    picked = [r["terms"].reshape(K, B, 3)[r["best"], np.arange(B), 1] for r in runs]
    assert (picked[1] < picked[0]).all(), picked


@pytest.mark.parametrize("name", lc.ORDER)
def test_every_gpu_case_keeps_its_decision_margins_and_both_dtypes_decide_alike(name):
    _, r32, r64, m32, m64 = lc.reference(name)
    assert m64.min >= lc.MIN_MARGIN, m64.by_kind
    assert m32.same_decisions(m64)
    assert (r32["steps"] == r64["steps"]).all() and (r32["best"] == r64["best"]).all()
    assert np.isfinite(r64["z"]).all() and np.abs(r64["z"]).max() < 100.0


def test_the_cases_cover_what_they_are_listed_for():
    c = lc.CASES
    assert {v[0] for v in c.values()} >= {1, 12, 70, 130}
    assert any(len(v[1]) + 1 == 2 and len(v[2]) + 1 == 4 for v in c.values())
    assert {w for v in c.values() for w in v[1] + v[2]} >= {1, 65, 512}
    assert {v[3] for v in c.values()} >= {1, 5} and {v[4] for v in c.values()} >= {1, 3}
    assert any(v[5] > 0 for v in c.values())
    assert {v[6] for v in c.values()} >= {0, 1, 5, 130}
    assert c["global_weights"][1] == [512, 512, 512] and c["global_weights"][7] == 3
    assert all(v[7] <= 25 for v in c.values())
    assert {v[9] for v in c.values()} >= {0.0, 0.9}
    steps = {n: lc.reference(n)[2]["steps"] for n in ("delta_at_0", "delta_mid", "half12_normal")}
    assert (steps["delta_at_0"] == 0).all() and (steps["half12_normal"] == 25).all()
    mid = steps["delta_mid"]
    assert ((mid > 0) & (mid < 25)).any() and (mid == 25).any()
    assert (lc.reference("delta_mid")[2]["best"] != 0).any()


def test_header_binding_and_build_list_carry_the_two_entries():
    from ggpm_amd import _lib, build
    assert "latent_search.hip" in build.SOURCES and "head_walk.h" in build.HEADERS
    text = open(os.path.join(ROOT, "include", "ggpm_hip.h")).read()
    for name, n_args in (("ggpm_latent_search_guided", 29), ("ggpm_latent_search_select", 12)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1])
