"""Synthetic step sequences for the atom level's decode loops (csrc/decode.hip) and a plain torch oracle of what they compute.

The loops take the tables ``ggpm_decode_steps`` names (include/ggpm_hip.h, "The atom level's decode loop as ONE call per
direction").  ``sequence()`` hand-builds a small level and T steps on it and ``tables()`` derives exactly those tables, by the
conventions of ``AtomPlan.__init__`` / ``AtomPlan.compact_tables`` (ggpm_amd/atom_decode.py) but without an ``AtomPlan``, a
schedule or a GPU: row 0 of the level is the null row; a step's sorted local row set is its recomputed (live) rows, the
frozen rows they read and row 0; ``frozen`` marks every row that is not live, padded with ones to a multiple of 16 bytes;
the local predecessor CSR has entries for live rows only; ``srcF[t][i]`` is the F id (foff[t'] + local row) of the last
earlier step t' that recomputed the level row, -1 if none did, for live rows and for row 0; ``srcH`` is the same look-up as
a row of the stacked [depth + 1][n] state blocks.

The step sizes and the forced rows are chosen for the properties tests/test_decode_steps_cases_cpu.py asserts on the
tables: one partial row tile, exactly one tile, one row into a second and into a third tile, a step whose frozen rows have
no producer, a frozen row two later steps read (two scatter-adds in different launches), a level row two steps recompute
(later readers see the second), live rows without predecessors, with frozen predecessors only, and reading another live
row of their step.

``oracle(case, dtype)`` restates the loops per depth with the formulas the header gives for the GRU and LSTM message
functions: start state F[srcF] on frozen rows and zero elsewhere, frozen rows kept for ``depth`` iterations, the final
states of the step's n rows to F rows foff[t] .. (LSTM: h and c); loss = sum(w_h F_h) (+ sum(w_c F_c)).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import level_form_cases as L

I, K = L.I, L.K
# local rows per step: 17 = one row into a second tile, 2 = the null row + one bond, 16 = exactly one tile, 33 = one row
# into a third tile, 15 = one partial tile, 70 = the largest step; T = 7
SIZES = (17, 2, 16, 33, 15, 70, 16)
GROUPS = {300: 5, 250: 4, 600: 10}        # column groups of a sparse call of these sizes (tg 4); H = 300 and 600: last group ragged
X_SCALE = 0.5                             # gate-input planes: 0.5 * standard_normal

Case = namedtuple("Case", "cell H depth")
CASES = [Case(cell, H, depth) for cell, Hs in (("GRU", (300, 250, 600)), ("LSTM", (300, 250))) for H in Hs
         for depth in (2, 3)]


def case_id(c):
    return "%s-H%d-d%d" % (c.cell, c.H, c.depth)


def gates(cell):
    return 4 if cell == "LSTM" else 3


def hidden_names(cell):
    """the hidden-half matrices in the order the loops take them (W of ggpm_decode_steps_forward)"""
    return ("Wi_h", "Wo_h", "Wu_h", "Wf_h") if cell == "LSTM" else ("Wz_h", "Ur", "Wh_h")


# ----------------------------------------------------------------------------- the step sequence
@lru_cache(maxsize=None)
def sequence(sizes=SIZES, seed=11):
    """-> (M, [(live level rows, {live row: [predecessor level rows]})] per step), deterministic.

    Fresh level rows are handed out in shuffled id order, so live and frozen rows interleave in a step's sorted row set.
    Forced rows (x, y, z are live rows of step 0):
      step 1 recomputes x alone, without predecessors (n = 2);
      steps 2 and 3 both read x (after its second producer) and y (two scatter-adds to y's F row of step 0);
      step 3 recomputes z, step 6 reads it (after its second producer).
    In every step with three live rows and a frozen one: the first live row reads frozen rows only, the second reads the
    first, the third reads nothing; every frozen row is read by some live row (that is what puts it into the row set)."""
    rs = np.random.RandomState(seed)
    M = 1 + 2 * sum(sizes)
    pool = [int(v) for v in rs.permutation(np.arange(1, M))]
    fresh = lambda k: [pool.pop() for _ in range(k)]
    steps, computed = [], []
    x = y = z = None
    for t, n in enumerate(sizes):
        nf = 0 if n == 2 else (n - 1) // 3
        nl = n - 1 - nf
        forced_live, forced_frozen = [], []
        if t == 1:
            forced_live = [x]
        if t in (2, 3):
            forced_frozen = [x, y]
        if t == 3:
            forced_live = [z]
        if t == 6:
            forced_frozen = [z]
        live = forced_live + fresh(nl - len(forced_live))
        cand = [r for r in computed if r not in live and r not in forced_frozen]
        take = min(len(cand), nf - len(forced_frozen))
        frozen = forced_frozen + [cand[i] for i in rs.permutation(len(cand))[:take]]
        frozen += fresh(nf - len(frozen))                    # (rows no step has computed: their state is zero)
        live = [live[i] for i in rs.permutation(len(live))]
        preds = {e: [] for e in live}
        special = nl >= 3 and nf >= 1
        readers = [e for e in live if not special or e != live[2]]
        for f in frozen:
            preds[readers[rs.randint(len(readers))]].append(f)
        if special:
            e0, e1 = live[0], live[1]
            preds[e0] += [f for f in frozen[:2] if f not in preds[e0]]
            preds[e1].append(e0)
        for e in (live[3:] if special else ()):
            others = [r for r in live + frozen if r != e and r not in preds[e]]
            extra = max(0, rs.randint(0, K + 1) - len(preds[e]))
            preds[e] += [others[i] for i in rs.permutation(len(others))[:extra]]
        if t == 0:
            x, y, z = live[3], live[4], live[5]
        steps.append((tuple(live), {e: tuple(p) for e, p in preds.items()}))
        computed += [e for e in live if e not in computed]
    return M, tuple(steps)


def _transpose(rows, cols, ncols):
    """(row, col) entry lists -> CSR of the transpose, entries of a row ascending"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((rows, cols))
    return (np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=ncols))]).astype(np.int32),
            rows[order].astype(np.int32))


@lru_cache(maxsize=None)
def tables(depth, sizes=SIZES, seed=11):
    """-> dict of the host tables of ``ggpm_decode_steps`` for the sequence (per-step lists of numpy arrays, the offsets as
    int64 arrays of length T + 1) plus ``rows`` (local -> level row), ``M`` and ``Ftot``"""
    M, steps = sequence(sizes, seed)
    T = len(steps)
    tb = dict(M=M, T=T, rows=[], frozen=[], pred_rowptr=[], pred_col=[], succ_rowptr=[], succ_col=[], srcF=[], srcH=[])
    for live, preds in steps:
        read = [p for e in live for p in preds[e]]
        rows = np.union1d(np.union1d(live, read), [0]).astype(np.int64)
        n = len(rows)
        lpos = np.full(M, -1, dtype=np.int64)
        lpos[rows] = np.arange(n)
        order = sorted(live)
        counts = np.zeros(n, dtype=np.int64)
        counts[lpos[order]] = [len(preds[e]) for e in order]
        flat = lpos[np.asarray([p for e in order for p in preds[e]], dtype=np.int64)]
        tb["pred_rowptr"].append(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
        tb["pred_col"].append(flat.astype(np.int32))
        rpT, colT = _transpose(np.repeat(lpos[order], [len(preds[e]) for e in order]), flat, n)
        tb["succ_rowptr"].append(rpT)
        tb["succ_col"].append(colT)
        fl = np.ones((n + 15) // 16 * 16, dtype=np.uint8)
        fl[lpos[order]] = 0
        tb["frozen"].append(fl)
        tb["rows"].append(rows)
    n = np.asarray([len(r) for r in tb["rows"]], dtype=np.int64)
    foff = np.concatenate([[0], np.cumsum(n)])
    stepof = np.repeat(np.arange(T), n)
    Hid = (depth + 1) * foff[stepof] + depth * n[stepof] + (np.arange(foff[-1]) - foff[stepof])
    last = np.full(M, -1, dtype=np.int64)
    for t in range(T):
        rows, fl = tb["rows"][t], tb["frozen"][t][:n[t]]
        sf = np.where(fl == 1, last[rows], -1)
        tb["srcF"].append(sf.astype(np.int32))
        tb["srcH"].append(np.where(sf >= 0, Hid[np.maximum(sf, 0)], -1).astype(np.int32))
        livepos = np.nonzero(fl == 0)[0]
        last[rows[livepos]] = foff[t] + livepos
    tb.update(n=n.astype(np.int32), foff=foff, roff=np.concatenate([[0], np.cumsum(depth * n)]),
              qoff=np.concatenate([[0], np.cumsum((depth + 1) * n)]), Ftot=int(foff[-1]), depth=depth)
    return tb


# ----------------------------------------------------------------------------- inputs
def _seed(case):
    return 1000 + 7 * case.H + 3 * case.depth + (1 if case.cell == "LSTM" else 0)


def weights(case):
    """the cell's full state dict, drawn as level_form_cases.weights draws it; the loops read the hidden halves"""
    from ggpm_amd.params import rnn_param_shapes, seeded_state_dict
    return seeded_state_dict(rnn_param_shapes(case.cell, I, case.H), seed=_seed(case))


def hidden_halves(case, sd):
    """-> ({name: [H, H] hidden-half matrix} in ``hidden_names`` order, b_u or None)"""
    if case.cell == "GRU":
        return ({"Wz_h": sd["W_z.weight"][:, I:], "Ur": sd["U_r.weight"], "Wh_h": sd["W_h.weight"][:, I:]},
                sd["U_r.bias"])
    return ({"Wi_h": sd["W_i.0.weight"][:, I:], "Wo_h": sd["W_o.0.weight"][:, I:], "Wu_h": sd["W.0.weight"][:, I:],
             "Wf_h": sd["W_f.0.weight"][:, I:]}, None)


@lru_cache(maxsize=None)
def inputs(case):
    """-> dict: ``X`` the gate-input planes in the layout of X_all without the pad columns ([G * Ftot, H]: step t's
    [G][n][H] block at row G * foff[t]), ``w_h`` / ``w_c`` the cotangents [Ftot, H], ``sd`` the weights"""
    tb = tables(case.depth)
    rs = np.random.RandomState(_seed(case) + 1)
    G, Ftot = gates(case.cell), tb["Ftot"]
    return dict(X=(X_SCALE * rs.standard_normal((G * Ftot, case.H))).astype(np.float32),
                w_h=rs.standard_normal((Ftot, case.H)).astype(np.float32),
                w_c=rs.standard_normal((Ftot, case.H)).astype(np.float32), sd=weights(case))


# ----------------------------------------------------------------------------- the oracle
def pred_table(rowptr, col, n):
    """local CSR -> [n, kmax] table padded with local row 0, the null row, whose state is zero throughout"""
    cnt = np.diff(rowptr)
    tab = np.zeros((n, max(1, int(cnt.max()))), dtype=np.int64)
    for r in np.nonzero(cnt)[0]:
        tab[r, :cnt[r]] = col[rowptr[r]:rowptr[r + 1]]
    return torch.from_numpy(tab)


def gru_step(W, bu, X, h, live, tab, depth):
    """include/ggpm_hip.h, "GRU message function", per depth; frozen rows (``live`` false) keep their state"""
    Wz, Ur, Wh = W
    Xz, Xr, Xh = X
    for _ in range(depth):
        q = h @ Ur.t() + bu
        hn = h[tab]
        s = hn.sum(dim=1)
        g = (torch.sigmoid(Xr.unsqueeze(1) + q[tab]) * hn).sum(dim=1)
        z = torch.sigmoid(Xz + s @ Wz.t())
        m = torch.tanh(Xh + g @ Wh.t())
        h = torch.where(live.unsqueeze(1), (1 - z) * s + z * m, h)
    return h


def lstm_step(W, X, h, c, live, tab, depth):
    """include/ggpm_hip.h, "LSTM message function", per depth"""
    Wi, Wo, Wu, Wf = W
    Xi, Xo, Xu, Xf = X
    for _ in range(depth):
        qf = h @ Wf.t()
        s = h[tab].sum(dim=1)
        fc = (torch.sigmoid(Xf.unsqueeze(1) + qf[tab]) * c[tab]).sum(dim=1)
        i = torch.sigmoid(Xi + s @ Wi.t())
        o = torch.sigmoid(Xo + s @ Wo.t())
        u = torch.tanh(Xu + s @ Wu.t())
        cn = i * u + fc
        h, c = torch.where(live.unsqueeze(1), o * torch.tanh(cn), h), torch.where(live.unsqueeze(1), cn, c)
    return h, c


def start_state(Fs, srcF, n, H, dtype):
    """F[srcF] where srcF >= 0, zero elsewhere"""
    src = torch.from_numpy(np.asarray(srcF, dtype=np.int64))
    if not Fs or not bool((src >= 0).any()):
        return torch.zeros(n, H, dtype=dtype)
    Fcat = torch.cat(Fs)
    return torch.where((src >= 0).unsqueeze(1), Fcat[src.clamp(min=0)], torch.zeros(n, H, dtype=dtype))


def run_oracle(case, dtype, tb=None):
    """-> dict of numpy arrays: F_h (F_c), dF (dCF) = the total gradient that reaches each F row, dX in the layout of
    ``inputs(case)["X"]``, the hidden-half weight gradients d<name> and, GRU, dbu"""
    tb = tables(case.depth) if tb is None else tb
    inp = inputs(case)
    lstm, G, H, depth = case.cell == "LSTM", gates(case.cell), case.H, case.depth
    halves, bu = hidden_halves(case, inp["sd"])
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)
    W = [leaf(halves[k]) for k in hidden_names(case.cell)]
    bu = leaf(bu) if bu is not None else None
    X = leaf(inp["X"])
    w_h, w_c = torch.from_numpy(inp["w_h"]).to(dtype), torch.from_numpy(inp["w_c"]).to(dtype)
    Fh, Fc, loss = [], [], 0
    for t in range(tb["T"]):
        n, f0 = int(tb["n"][t]), int(tb["foff"][t])
        live = torch.from_numpy(tb["frozen"][t][:n] == 0)
        tab = pred_table(tb["pred_rowptr"][t], tb["pred_col"][t], n)
        Xt = X[G * f0:G * (f0 + n)].view(G, n, H)
        h = start_state(Fh, tb["srcF"][t], n, H, dtype)
        if lstm:
            h, c = lstm_step(W, Xt, h, start_state(Fc, tb["srcF"][t], n, H, dtype), live, tab, depth)
            c.retain_grad()
            Fc.append(c)
            loss = loss + (w_c[f0:f0 + n] * c).sum()
        else:
            h = gru_step(W, bu, Xt, h, live, tab, depth)
        h.retain_grad()
        Fh.append(h)
        loss = loss + (w_h[f0:f0 + n] * h).sum()
    loss.backward()
    cat = lambda ts: torch.cat([v.detach() for v in ts]).numpy()
    out = dict(F_h=cat(Fh), dF=torch.cat([v.grad for v in Fh]).numpy(), dX=X.grad.numpy())
    if lstm:
        out.update(F_c=cat(Fc), dCF=torch.cat([v.grad for v in Fc]).numpy())
    else:
        out["dbu"] = bu.grad.numpy()
    out.update({"d" + k: w.grad.numpy() for k, w in zip(hidden_names(case.cell), W)})
    return out


@lru_cache(maxsize=None)
def oracle(case, dtype):
    """``run_oracle`` on the case's own tables, computed once per (case, dtype) and shared: do not write to the arrays"""
    return run_oracle(case, dtype)
