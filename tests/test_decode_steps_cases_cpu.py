"""CPU: the synthetic decode-step sequences of tests/decode_steps_cases.py have the properties they were built for, their
oracle agrees with oracle/ref_encoder.py on a single step to fp64 rounding, its own fp32 run stays below the 1e-4 bar on
every case, and every step size takes the column-grouped fp32-MFMA form of the smallest sparse class."""
import numpy as np
import pytest
import torch

import decode_steps_cases as D
from golden_utils import rel_err


def _tables():
    return D.tables(2)


def _live(tb, t):
    n = int(tb["n"][t])
    return tb["frozen"][t][:n] == 0


def _brute_srcF(tb, t, i):
    """F id of the last step before t that recomputed local row i's level row, by scanning the steps backwards"""
    row = tb["rows"][t][i]
    for u in range(t - 1, -1, -1):
        pos = np.nonzero(tb["rows"][u] == row)[0]
        if len(pos) and _live(tb, u)[pos[0]]:
            return int(tb["foff"][u] + pos[0])
    return -1


def _step_of(tb, fid):
    return int(np.searchsorted(tb["foff"], fid, side="right") - 1)


def test_step_sizes_cover_the_row_tile_edges():
    tb = _tables()
    n = tb["n"].tolist()
    assert n == list(D.SIZES) and 6 <= tb["T"] <= 8
    assert {2, 15, 16, 17, 33} <= set(n) and max(n) == 70


@pytest.mark.parametrize("depth", (2, 3))
def test_tables_follow_the_conventions_of_the_atom_plan(depth):
    tb = D.tables(depth)
    T, n = tb["T"], tb["n"].astype(np.int64)
    assert tb["foff"].tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
    assert tb["roff"].tolist() == np.concatenate([[0], np.cumsum(depth * n)]).tolist()
    assert tb["qoff"].tolist() == np.concatenate([[0], np.cumsum((depth + 1) * n)]).tolist()
    for t in range(T):
        rows, fl, live = tb["rows"][t], tb["frozen"][t], _live(tb, t)
        assert rows[0] == 0 and (np.diff(rows) > 0).all() and rows[-1] < tb["M"]
        assert len(fl) % 16 == 0 and len(fl) - n[t] < 16 and fl[0] == 1 and (fl[n[t]:] == 1).all()
        rp, col = tb["pred_rowptr"][t], tb["pred_col"][t]
        assert rp[0] == 0 and rp[-1] == len(col) and len(rp) == n[t] + 1
        assert (np.diff(rp)[~live] == 0).all()                       # only live rows have entries
        assert ((col > 0) & (col < n[t])).all()                      # never the null row, never out of the step
        # every frozen row but the null row is there because a live row reads it
        assert set(np.nonzero(~live)[0].tolist()) - {0} <= set(col.tolist())
        # the transpose, entries ascending
        srp, scol = tb["succ_rowptr"][t], tb["succ_col"][t]
        ent = sorted((int(c), r) for r in range(n[t]) for c in col[rp[r]:rp[r + 1]])
        assert [(c, int(r)) for c in range(n[t]) for r in scol[srp[c]:srp[c + 1]]] == ent
        # srcF / srcH: the last earlier producer, resolved independently
        sf, sh = tb["srcF"][t], tb["srcH"][t]
        assert len(sf) == len(sh) == n[t]
        for i in range(n[t]):
            want = -1 if live[i] or i == 0 else _brute_srcF(tb, t, i)
            assert sf[i] == want, (t, i)
            if want < 0:
                assert sh[i] == -1
            else:
                u = _step_of(tb, want)
                assert u < t and sh[i] == tb["qoff"][u] + depth * n[u] + (want - tb["foff"][u])
        pos = sf[sf >= 0]
        assert len(set(pos.tolist())) == len(pos)                    # unique within the step


def test_a_step_whose_frozen_rows_have_no_producer():
    tb = _tables()
    assert any((tb["srcF"][t] < 0).all() and (~_live(tb, t)).sum() > 1 for t in range(tb["T"]))


def test_a_frozen_row_is_read_by_two_later_steps():
    tb = _tables()
    readers = {}
    for t in range(tb["T"]):
        for f in tb["srcF"][t][tb["srcF"][t] >= 0].tolist():
            readers.setdefault(f, set()).add(t)
    assert any(len(s) >= 2 for s in readers.values())


def test_a_row_recomputed_twice_is_read_from_its_second_producer():
    tb = _tables()
    hits = 0
    for t in range(tb["T"]):
        for i in np.nonzero(tb["srcF"][t] >= 0)[0]:
            row = tb["rows"][t][i]
            prod = [u for u in range(t) if row in tb["rows"][u] and _live(tb, u)[np.nonzero(tb["rows"][u] == row)[0][0]]]
            if len(prod) >= 2:
                assert _step_of(tb, tb["srcF"][t][i]) == prod[-1]
                hits += 1
    assert hits >= 2


def test_live_rows_of_every_kind():
    tb = _tables()
    none = all_frozen = live_live = 0
    for t in range(tb["T"]):
        live, rp, col = _live(tb, t), tb["pred_rowptr"][t], tb["pred_col"][t]
        for r in np.nonzero(live)[0]:
            p = col[rp[r]:rp[r + 1]]
            none += len(p) == 0
            all_frozen += len(p) > 0 and not live[p].any()
            live_live += bool(live[p].any())
    assert none >= 1 and all_frozen >= 1 and live_live >= 1


def test_every_step_size_takes_the_smallest_column_grouped_form():
    """host only: tg 4 on fp32 MFMA, one row tile per workgroup, 4 / 5 / 10 column groups (H = 300: 19 tiles, the last
    group holds three; H = 600: 38 tiles, the last group holds two), with B launches in both directions"""
    from ggpm_amd import functional as F_
    for case in D.CASES:
        for n in sorted(set(D.SIZES)):
            form = F_.level_form(case.cell == "LSTM", n, case.H, sparse=True)
            assert form is not None
            assert (form.tg, form.groups, form.gate_mode, form.rt2) == (4, D.GROUPS[case.H], 0, 0), (case, n)
            assert form.Hp == (case.H + 15) // 16 * 16 and form.tiles == form.Hp // 16
            assert form.tiles % form.tg == {300: 3, 250: 0, 600: 2}[case.H]      # tiles of the last group (0: a full one)
            assert (form.fuse_fwd, form.fuse_bwd) == (0, 0)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_oracle_fp32_run_stays_below_the_bar(case):
    """the inputs are scaled so that the oracle's own fp32 run is well inside 1e-4 of fp64 on every compared tensor"""
    w64, w32 = D.oracle(case, torch.float64), D.oracle(case, torch.float32)
    assert sorted(w64) == sorted(w32)
    for k in w64:
        assert np.isfinite(w64[k]).all() and np.abs(w64[k]).max() > 0, k
        assert rel_err(w32[k], w64[k]) < 1e-4, (k, rel_err(w32[k], w64[k]))
    tb = D.tables(case.depth)
    for t in range(tb["T"]):              # the null row stays zero
        assert (w64["F_h"][tb["foff"][t]] == 0).all()


@pytest.mark.parametrize("cell", ("GRU", "LSTM"))
def test_one_step_agrees_with_the_reference_cell_in_fp64(cell):
    """One step of the restated oracle against oracle/ref_encoder.py's sparse_forward in fp64: the gate inputs formed from
    an x and the input halves, the new state and the gradients of the incoming state, of x and of the hidden halves,
    each to 1e-12 (two fp64 evaluations of one formula)."""
    from oracle import ref_encoder as ref
    case = D.Case(cell, 300, 3)
    tb = D.tables(case.depth)
    t = 3                                  # 33 rows, frozen rows with and without a producer, every kind of live row
    n, H, dt = int(tb["n"][t]), case.H, torch.float64
    live = _live(tb, t)
    rs = np.random.RandomState(5)
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)
    sd = D.weights(case)
    p = {"rnn." + k: leaf(v) for k, v in sd.items()}
    x, h_in, c_in = leaf(rs.standard_normal((n, D.I))), leaf(rs.standard_normal((n, H))), leaf(rs.standard_normal((n, H)))
    w_h, w_c = (torch.from_numpy(rs.standard_normal((n, H))) for _ in range(2))
    tab = D.pred_table(tb["pred_rowptr"][t], tb["pred_col"][t], n)
    sub = torch.from_numpy(np.nonzero(live)[0])
    # the reference on the step's rows: row 0 is its pad row, which the level keeps at zero
    m0 = torch.ones(n, 1, dtype=dt)
    m0[0] = 0
    if cell == "GRU":
        rh = ref.gru_sparse_forward(p, "rnn.", h_in * m0, x[sub], sub, tab[sub], case.depth)
        (w_h * rh).sum().backward()
    else:
        rh, rc = ref.lstm_sparse_forward(p, "rnn.", h_in * m0, c_in * m0, x[sub], sub, tab[sub], case.depth)
        ((w_h * rh).sum() + (w_c * rc).sum()).backward()
    names = {"GRU": ("W_z", "U_r", "W_h"), "LSTM": ("W_i.0", "W_o.0", "W.0", "W_f.0")}[cell]
    hid = lambda g: g if g.shape[1] == H else g[:, D.I:]
    want = dict(h=rh.detach(), dh_in=h_in.grad.clone(), dx=x.grad.clone(),
                **{"dW%d" % k: hid(p["rnn." + nm + ".weight"].grad).clone() for k, nm in enumerate(names)})
    if cell == "LSTM":
        want.update(c=rc.detach(), dc_in=c_in.grad.clone())
    else:
        want["dbu"] = p["rnn.U_r.bias"].grad.clone()
    for v in list(p.values()) + [x, h_in, c_in]:
        v.grad = None
    # the restated step: gate inputs from x and the input halves, the masked start state
    fz = torch.from_numpy((~live).astype(np.float64)).unsqueeze(1) * m0
    if cell == "GRU":
        X = [x @ p["rnn.W_z.weight"][:, :D.I].t() + p["rnn.W_z.bias"], x @ p["rnn.W_r.weight"].t(),
             x @ p["rnn.W_h.weight"][:, :D.I].t() + p["rnn.W_h.bias"]]
        W = [p["rnn.W_z.weight"][:, D.I:], p["rnn.U_r.weight"], p["rnn.W_h.weight"][:, D.I:]]
        h = D.gru_step(W, p["rnn.U_r.bias"], X, h_in * fz, torch.from_numpy(live), tab, case.depth)
        (w_h * h).sum().backward()
    else:
        X = [x @ p["rnn.%s.weight" % nm][:, :D.I].t() + p["rnn.%s.bias" % nm] for nm in names]
        W = [p["rnn.%s.weight" % nm][:, D.I:] for nm in names]
        h, c = D.lstm_step(W, X, h_in * fz, c_in * fz, torch.from_numpy(live), tab, case.depth)
        ((w_h * h).sum() + (w_c * c).sum()).backward()
    got = dict(h=h.detach(), dh_in=h_in.grad, dx=x.grad,
               **{"dW%d" % k: hid(p["rnn." + nm + ".weight"].grad) for k, nm in enumerate(names)})
    if cell == "LSTM":
        got.update(c=c.detach(), dc_in=c_in.grad)
    else:
        got["dbu"] = p["rnn.U_r.bias"].grad
    assert sorted(got) == sorted(want)
    for k in want:
        assert float(want[k].abs().max()) > 0, k
        assert rel_err(got[k].numpy(), want[k].numpy()) < 1e-12, (k, rel_err(got[k].numpy(), want[k].numpy()))
    # only the frozen rows pass a gradient to the incoming state
    assert float(got["dh_in"][torch.from_numpy(live)].abs().max()) == 0.0
