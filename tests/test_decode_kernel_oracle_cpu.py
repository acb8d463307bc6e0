"""CPU: the fp64 restatements the greedy-decode kernel tests compare against (tests/decode_kernel_oracle.py) are themselves
anchored -- the two top-k selections to outputs of the reference's own ``nnutils.hier_topk`` and of the root selection of
``MotifDecoder.decode`` (tests/golden/motif_decode_topk, made by tests/golden/make_golden_topk.py), the one-message form
of the sparse forward to the multi-row oracle that tests/test_oracle_golden.py pins."""
import numpy as np
import pytest
import torch

import decode_kernel_oracle as O


def test_fixture_cases_are_recorded():
    have = set(O.topk_fixture_names())
    assert {"c300_i900_k5", "c40_i130_k16"} <= have and 3 <= len(have) <= 4, have


@pytest.mark.parametrize("name", O.topk_fixture_names())
def test_topk_restatement_reproduces_the_reference(name):
    g = O.TopkGolden(name)
    for mode, want, k, fn in (("hier", g.hier, g.k, O.hier_topk), ("root", g.root, g.k_root, O.root_topk)):
        ws, wc, wa = g.split(want, k)
        s, c, a, gap = fn(g.cls, g.icls, g.owner, k)
        assert np.array_equal(c, wc) and np.array_equal(a, wa), (name, mode)
        err = float(np.abs(s - ws).max())
        print("%s %s: scores within %.2e, smallest gap %.2e" % (name, mode, err, gap))
        assert err <= 1e-9, (name, mode, err)


@pytest.mark.parametrize("n_cls,n_icls,k,cap,seed", O.TOPK_CASES)
def test_seeded_cases_keep_their_gap(n_cls, n_icls, k, cap, seed):
    """the precondition of the kernel comparison holds for every hard-coded seed, and the owner table is ragged"""
    cls, icls, owner = O.topk_inputs(n_cls, n_icls, k, seed, cap=cap)
    assert O.hier_topk(cls, icls, owner, k)[3] >= O.MIN_GAP
    assert O.root_topk(cls, icls, owner, k)[3] >= O.MIN_GAP
    for rows in (cls, icls):           # any two raw scores of a row: 0.007 apart (less the fp32 rounding of the two)
        assert np.diff(np.sort(rows.astype(np.float64), axis=1), axis=1).min() >= 0.00699
    counts = np.bincount(owner, minlength=n_cls)
    assert (counts == 0).sum() == 1 and (counts == 1).sum() >= 1
    if cap is not None:
        assert counts.max() <= cap < 16
    elif n_icls >= 36:
        assert counts.max() > 16


def test_tie_rule_on_a_hand_made_row():
    cls, icls, owner, k, expected = O.tie_case()
    for mode, fn in (("hier", O.hier_topk), ("root", O.root_topk)):
        s, c, a, gap = fn(cls, icls, owner, k, ties=True)
        assert (c[0].tolist(), a[0].tolist()) == expected[mode], mode
        assert gap >= O.MIN_GAP
    s, c, a, _ = O.hier_topk(cls, icls, owner, k, ties=True)
    assert s[0, 0] == s[0, 1] and s[0, 2] == s[0, 3] == s[0, 4]          # exact ties, lower index first
    # a motif that owns fewer than k: its masked attachments follow by raw score, equal ones by index
    s, c, a, _ = O.root_topk(np.eye(300, dtype=np.float32)[3:4], icls, owner, 8, ties=True)
    assert a[0].tolist() == [7, 400, 401, 402, 3, 67, 259, 4] and c[0].tolist() == [3] * 8


@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_one_message_form_equals_the_multi_row_sparse_forward(rnn):
    """``tree_message`` (submess = [e]) on each of a set of independent messages = one sparse forward over all of them"""
    H, depth = 24, 2
    p = O.f64(O.decoder(rnn, H, 8, 50, 150).state_dict())
    st = O.tree_state(3, H)
    rows = st["mess"][:, 0]
    hn, cn = O.tree_messages(p, rnn, depth, st["h"], st["c"], st["fnode"], st["fmess"], st["bgraph"], rows)
    h0 = torch.from_numpy(st["h"]).double()
    untouched = np.setdiff1d(np.arange(st["E"]), rows)
    assert torch.equal(hn[untouched], h0[untouched])
    for e in rows:
        he, ce = O.tree_message(p, rnn, depth, st["h"], st["c"], st["fnode"], st["fmess"], st["bgraph"], int(e))
        assert float((he - hn[e]).abs().max()) <= 1e-12
        assert float(he.abs().max()) > 1e-3
        if rnn == "LSTM":
            assert float((ce - cn[e]).abs().max()) <= 1e-12
    assert sorted(set(st["cnt_mess"])) == sorted(O.NB_COUNTS)
    assert {0, O.MAX_POS - 1} <= set(st["fmess"][rows, 1].tolist())
