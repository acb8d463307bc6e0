"""CPU: the conditions under which tests/test_head_kernels_gpu.py compares the kernels with fp64 hold for its hard-coded
seeds -- so a change of a case or a seed there is caught without a GPU."""
import numpy as np

import property_oracle as po
import test_head_kernels_gpu as T


def test_attachment_head_decisions_have_a_margin_and_the_cases_mix_every_kind_of_prediction():
    for case in T.HEAD_ORDER:
        H, L, C, B, preds = T.HEAD_CASES[case]
        assert H + 20 <= 1024 and L <= 1024 and all(1 <= n <= C and k in (1, 2) and 0 <= nth < 20 and 0 <= b < B
                                                    for n, k, nth, b in preds)
        if len(preds) > 1:
            assert {k for _, k, _, _ in preds} == {1, 2}
            assert {1, C} <= {n for n, _, _, _ in preds} and {0, 19} <= {nth for _, _, nth, _ in preds}
        for distinct in (False, True):
            assert T.head_reference(case, distinct)[4] > 1e-4, (case, distinct)
    mols = [b for _, _, _, b in T.HEAD_CASES["d_H600"][4]]
    assert 3 not in mols and all(a != b for a, b in zip(mols, mols[1:])) and min(mols.count(b) for b in set(mols)) > 1


def test_property_head_cases_have_no_unit_at_its_kink():
    for i in range(len(T.HEADS_CASES)):
        for dropout in (0.0, 0.1):
            assert T.heads_reference(i, dropout)[5] > 1e-5, (i, dropout)


def test_latent_search_cases_have_margins_end_and_stay_bounded():
    for i in range(len(T.SEARCH_CASES)):
        _, _, _, runs, margin = T.search_reference(i)
        z64, _, n64, st64 = runs[np.float64]
        assert margin >= 1e-3 and (st64 == po.DONE).all() and np.abs(z64).max() < 100.0, i
        assert (runs[np.float32][2] == n64).all(), i
