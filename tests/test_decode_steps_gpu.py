"""GPU: the atom level's decode step loops (csrc/decode.hip) and the level options only they set, driven directly through
the C entry points on the synthetic sequences of tests/decode_steps_cases.py, against the fp64 oracle of that module.

Which test calls which entry point:
  ggpm_decode_steps_forward / _backward, ggpm_{gru,lstm}_weight_grads_stacked and
  ggpm_weight_grads_stacked_workspace_bytes      test_driver_matches_fp64 (and every test that uses ``_driver``)
  ggpm_decode_steps_infer                        test_forward_only_form_is_bit_identical
  the three _async forms, the worker thread and ggpm_decode_join
                                                 test_worker_thread_forms_are_bit_identical, test_worker_thread_error_path
  ggpm_level_opts.gather_* (folded start state), scatter_* (folded scatter-add), weights_packed, defer_stash
                                                 set by the drivers; test_folded_loop_is_bit_identical_to_public_calls issues the
                                                 same steps without gather_* / scatter_* / weights_packed
  ggpm_level_opts.h_out / c_out on a sparse forward
                                                 test_forward_only_form_is_bit_identical

Every buffer a call writes starts as NaN, with a NaN guard region behind it; only the cotangents (dF, dCF) and the last DQ
slot of every block (include/ggpm_hip.h: ggpm_level_opts.defer_stash) hold numbers.  Both bars of
tests/test_gpu_level_forms.py::_check apply: 1e-4, and 3x (+1e-6) the oracle's own fp32 distance from fp64.
profiles/decode_steps.txt records the line each case printed."""
import ctypes
import time
from functools import lru_cache

import numpy as np
import pytest
import torch

import decode_steps_cases as D
import level_form_cases as C
from test_gpu_level_forms import _check

pytestmark = pytest.mark.gpu

GUARD = 8            # NaN rows behind every stacked buffer
SENTINEL = 12345.0   # what the outputs the deferred backward must leave alone are filled with
NAN = float("nan")


def _mods():
    from ggpm_amd import _lib, atom_decode
    from ggpm_amd import functional as F_
    return _lib, _lib.load(), F_, atom_decode


def _dev():
    return torch.device("cuda:0")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit for bit (NaN guards included)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


class Env:
    """What every run of a case shares: the tables on the device (one packed int32 upload and one byte upload, as AtomPlan
    keeps them, so that an empty table still has an address), the descriptor, the cell adapter with the weights, X_all and
    the cotangents."""

    def __init__(self, case):
        _lib, lib, F_, atom_decode = _mods()
        tb, inp = D.tables(case.depth), D.inputs(case)
        self.case, self.tb = case, tb
        self.lstm, self.G, self.H, self.depth = case.cell == "LSTM", D.gates(case.cell), case.H, case.depth
        self.Hp, self.T, self.Ftot = F_.padded_hidden(case.H), tb["T"], tb["Ftot"]
        self.n = [int(v) for v in tb["n"]]
        self.nmax = max(self.n)
        self.foff, self.roff, self.qoff = ([int(v) for v in tb[k]] for k in ("foff", "roff", "qoff"))
        self.R, self.Q = self.roff[-1], self.qoff[-1]
        dev = _dev()
        names = ("srcH", "srcF", "pred_rowptr", "pred_col", "succ_rowptr", "succ_col")
        parts, off, fill = [], {}, 0
        for k in names:
            for t in range(self.T):
                off[k, t] = fill
                fill += len(tb[k][t])
                parts.append(np.asarray(tb[k][t], dtype=np.int32))
        parts.append(np.zeros(4, dtype=np.int32))
        self.ints = torch.from_numpy(np.concatenate(parts)).to(dev)
        self.ptr = {key: self.ints.data_ptr() + 4 * o for key, o in off.items()}
        foffs = np.concatenate([[0], np.cumsum([len(f) for f in tb["frozen"]])])
        self.frozen = torch.from_numpy(np.concatenate(tb["frozen"])).to(dev)
        for t in range(self.T):
            self.ptr["frozen", t] = self.frozen.data_ptr() + int(foffs[t])
        self.desc, self._keep = self.descriptor(self.T)
        sd = inp["sd"]
        if self.lstm:       # the parameter order of rnn.LSTM.level_params / rnn.GRU.level_params
            params = tuple(torch.from_numpy(sd[g + sfx]).to(dev) for g in ("W_i.0", "W_o.0", "W.0", "W_f.0")
                           for sfx in (".weight", ".bias"))
        else:
            params = tuple(torch.from_numpy(sd[k]).to(dev) for k in ("W_z.weight", "W_z.bias", "W_r.weight", "U_r.weight",
                                                                     "U_r.bias", "W_h.weight", "W_h.bias"))
        self.cell = F_.cell_for(self.lstm, params, D.I, self.H)
        self.W_arr, self.ld_arr = self.cell.hidden_weight_arrays()       # as atom_decode._compact_prelude hands them over
        self.bu = self.cell.b_u
        pad = lambda a: torch.nn.functional.pad(torch.from_numpy(a), (0, self.Hp - self.H)).to(dev)
        self.X_all = pad(inp["X"])                                        # [G * Ftot, Hp], pad columns zero
        self.w_h, self.w_c = pad(inp["w_h"]), pad(inp["w_c"])
        fn = lib.ggpm_lstm_backward_workspace_bytes if self.lstm else lib.ggpm_gru_backward_workspace_bytes
        self._work_floats = (int(fn(self.nmax, self.H, self.depth)) + 3) // 4
        self.form = F_.level_form(self.lstm, self.nmax, self.H, sparse=True)
        self.check_case = C.Case(case.cell, case.H, self.nmax, case.depth, None, True, 0)

    def descriptor(self, T):
        """ggpm_decode_steps over the first T steps (T = 0: the descriptor the entry points refuse)"""
        _lib, _, _, atom_decode = _mods()
        tb, Tn = self.tb, self.T
        keep = dict(n=_lib.array_type(ctypes.c_int32, Tn)(*self.n))
        for k in ("foff", "roff", "qoff"):
            keep[k] = _lib.array_type(ctypes.c_int64, Tn + 1)(*[int(v) for v in tb[k]])
        for k in ("srcH", "srcF", "frozen", "pred_rowptr", "pred_col", "succ_rowptr", "succ_col"):
            keep[k] = _lib.array_type(ctypes.c_void_p, Tn)(*[self.ptr[k, t] for t in range(Tn)])
        fields = ("n", "foff", "roff", "qoff", "srcH", "srcF", "frozen", "pred_rowptr", "pred_col", "succ_rowptr", "succ_col")
        d = atom_decode.DecodeSteps(T, self.H, self.depth, int(self.lstm), *[ctypes.addressof(keep[k]) for k in fields])
        return d, keep

    # ---- buffers: NaN wherever a call writes, a NaN guard behind each
    def forward_buffers(self):
        Hp, g = self.Hp, GUARD
        return dict(Hs=_nan(self.Q + g, Hp), Cs=_nan(self.Q + g, Hp) if self.lstm else None, Qs=_nan(self.R + g, Hp),
                    St=_nan(5, self.R + g, Hp), wpack=_nan(self.cell.pack_floats() + g * Hp), tmp=_nan(2 * self.nmax + g, Hp))

    def infer_buffers(self):
        Hp, g, m = self.Hp, GUARD, 2 * self.nmax
        return dict(F_h=_nan(self.Ftot + g, Hp), F_c=_nan(self.Ftot + g, Hp) if self.lstm else None, Hs=_nan(m + g, Hp),
                    Cs=_nan(m + g, Hp) if self.lstm else None, Qs=_nan(m + g, Hp), wpack=_nan(self.cell.pack_floats() + g * Hp))

    def work_floats(self):
        """floats of the backward workspace of the largest step, sized by the library"""
        return self._work_floats

    def backward_buffers(self, cotangent=True):
        """``cotangent`` False: dF / dCF and DQ stay NaN too (calls that must launch nothing)"""
        Hp, g, H = self.Hp, GUARD, self.H
        b = dict(dF=_nan(self.Ftot + g, Hp), dCF=_nan(self.Ftot + g, Hp) if self.lstm else None,
                 dX=_nan(self.G * self.Ftot + g, Hp), DG=_nan(3 if self.lstm else 2, self.R + g, Hp), DQ=_nan(self.Q + g, Hp),
                 work=_nan(self.work_floats() + g * Hp), tmp=_nan(2 * self.nmax + g, Hp))
        # what a level call would write its weight gradients to: the deferred backward leaves them alone (GRU: [3] = b_u)
        b["dW_unused"] = [torch.full((H, H) if self.lstm or k < 3 else (H,), SENTINEL, device=_dev()) for k in range(4)]
        if cotangent:
            b["dF"][:self.Ftot] = self.w_h                   # dF carries the cotangent
            if self.lstm:
                b["dCF"][:self.Ftot] = self.w_c
            for t in range(self.T):                          # the last DQ slot of every block lines up with Hs: zero
                b["DQ"][self.qoff[t] + self.depth * self.n[t]:self.qoff[t + 1]] = 0
        return b

    # ---- the C calls
    def forward(self, b, fn="ggpm_decode_steps_forward", desc=None, X=True, Cs=True, bu=True):
        _lib, lib, F_, _ = _mods()
        P = F_._p
        return getattr(lib, fn)(ctypes.byref(self.desc if desc is None else desc), self.W_arr, self.ld_arr,
                                P(self.bu) if bu else None, P(self.X_all) if X else None, P(b["Hs"]),
                                P(b["Cs"]) if Cs else None, P(b["Qs"]), P(b["St"]), b["St"].stride(0), P(b["wpack"]),
                                P(b["tmp"]), F_._stream())

    def infer(self, b, fn="ggpm_decode_steps_infer", desc=None, X=True, Cs=True, bu=True):
        _lib, lib, F_, _ = _mods()
        P = F_._p
        return getattr(lib, fn)(ctypes.byref(self.desc if desc is None else desc), self.W_arr, self.ld_arr,
                                P(self.bu) if bu else None, P(self.X_all) if X else None, P(b["F_h"]), P(b["F_c"]), P(b["Hs"]),
                                P(b["Cs"]) if Cs else None, P(b["Qs"]), P(b["wpack"]), F_._stream())

    def backward(self, f, b, fn="ggpm_decode_steps_backward", desc=None, X=True, Cs=True, work_bytes=None):
        _lib, lib, F_, _ = _mods()
        P = F_._p
        b["dW_arr"] = _lib.array_type(ctypes.c_void_p, 4)(*[a.data_ptr() for a in b["dW_unused"]])
        return getattr(lib, fn)(ctypes.byref(self.desc if desc is None else desc), self.W_arr, self.ld_arr,
                                P(self.X_all) if X else None, P(f["Hs"]), P(f["Cs"]) if Cs else None, P(f["Qs"]), P(f["St"]),
                                f["St"].stride(0), P(b["dF"]), P(b["dCF"]), P(b["dX"]), P(b["DG"]), b["DG"].stride(0),
                                P(b["DQ"]), b["dW_arr"], P(b["work"]),
                                self.work_floats() * 4 if work_bytes is None else work_bytes, P(b["tmp"]), F_._stream())

    def weight_grads(self, f, b):
        """ggpm_*_weight_grads_stacked over the stacked stashes, as atom_decode's tail calls it -> {name: gradient}"""
        _lib, lib, F_, _ = _mods()
        P, H, R, Q = F_._p, self.H, self.R, self.Q
        wsb = int(lib.ggpm_weight_grads_stacked_workspace_bytes(H, max(R, Q)))
        ws = _nan((wsb + 3) // 4 + GUARD)
        names = D.hidden_names(self.case.cell)
        out = {"d" + k: _nan(H + GUARD, H) for k in names}
        St, DG = f["St"], b["DG"]
        if self.lstm:
            o = [out["d" + k] for k in names]
            rc = lib.ggpm_lstm_weight_grads_stacked(R, Q, H, P(DG[0]), P(DG[1]), P(DG[2]), P(St[0]), P(b["DQ"]), P(f["Hs"]),
                                                    P(o[0]), H, P(o[1]), H, P(o[2]), H, P(o[3]), H, P(ws), wsb, F_._stream())
        else:
            out["dbu"] = _nan(H + GUARD)
            rc = lib.ggpm_gru_weight_grads_stacked(R, Q, H, P(DG[0]), P(St[1]), P(DG[1]), P(St[0]), P(b["DQ"]), P(f["Hs"]),
                                                   P(out["dWz_h"]), H, P(out["dUr"]), H, P(out["dbu"]), P(out["dWh_h"]), H,
                                                   P(ws), wsb, F_._stream())
        assert rc == 0
        assert _all_nan(ws[(wsb + 3) // 4:])
        return out


@lru_cache(maxsize=None)
def _env(case):
    return Env(case)


def _run_driver(env):
    """forward, backward and the stacked contraction through the synchronous drivers on fresh buffers"""
    f, b = env.forward_buffers(), env.backward_buffers()
    assert env.forward(f) == 0
    assert env.backward(f, b) == 0
    wg = env.weight_grads(f, b)
    torch.cuda.synchronize()
    return f, b, wg


@lru_cache(maxsize=None)
def _driver(case):
    """the case's driver run, computed once and shared (read only)"""
    return _run_driver(_env(case))


def _guards_intact(env, f=None, b=None, wg=None):
    if f is not None:
        assert _all_nan(f["Hs"][env.Q:]) and _all_nan(f["Qs"][env.R:]) and _all_nan(f["St"][:, env.R:])
        assert f["Cs"] is None or _all_nan(f["Cs"][env.Q:])
        assert _all_nan(f["wpack"][env.cell.pack_floats():]) and _all_nan(f["tmp"][2 * env.nmax:])
    if b is not None:
        assert _all_nan(b["dF"][env.Ftot:]) and _all_nan(b["dX"][env.G * env.Ftot:]) and _all_nan(b["DG"][:, env.R:])
        assert _all_nan(b["DQ"][env.Q:]) and _all_nan(b["work"][env.work_floats():]) and _all_nan(b["tmp"][2 * env.nmax:])
        assert b["dCF"] is None or _all_nan(b["dCF"][env.Ftot:])
    for k, v in (wg or {}).items():
        assert _all_nan(v[env.H:]), k


def _final_rows(env, stacked):
    """slot ``depth`` of every block of a stacked state buffer = the F rows [Ftot, Hp]"""
    return torch.cat([stacked[env.qoff[t] + env.depth * env.n[t]:env.qoff[t + 1]] for t in range(env.T)])


def _got(env, f, b, wg):
    H, cpu = env.H, lambda t: t.cpu().numpy()
    got = dict(F_h=cpu(_final_rows(env, f["Hs"])[:, :H]), dF=cpu(b["dF"][:env.Ftot, :H]),
               dX=cpu(b["dX"][:env.G * env.Ftot, :H]))
    if env.lstm:
        got.update(F_c=cpu(_final_rows(env, f["Cs"])[:, :H]), dCF=cpu(b["dCF"][:env.Ftot, :H]))
    got.update({k: cpu(v[:H]) for k, v in wg.items()})
    return got


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_driver_matches_fp64(case):
    """ggpm_decode_steps_forward, _backward and the stacked weight-gradient contraction against the fp64 oracle under both
    bars: the F rows (slot ``depth`` of every block; LSTM: h and c), dX_all, dF / dCF after the loop (the total gradient
    of every F row: the check on the scatter-adds, the row two steps read included), every hidden-half weight gradient
    and db_u.  Prints the case's line."""
    t0 = time.perf_counter()
    env = _env(case)
    f, b, wg = _driver(case)
    _check(env.check_case, env.form, _got(env, f, b, wg), D.oracle(case, torch.float64), D.oracle(case, torch.float32), t0)
    for w in b["dW_unused"]:
        assert bool((w == SENTINEL).all())
    _guards_intact(env, f, b, wg)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_forward_state_blocks(case):
    """What the training forward leaves in the stacked buffers: slot 0 of every block is the gathered start state bit for
    bit (zero where srcH is -1), the null row and the pad columns are zero in every state slot, nothing the backward
    reads is NaN, the guards are intact."""
    env = _env(case)
    f, _, _ = _driver(case)
    n, depth, H, Hp = env.n, env.depth, env.H, env.Hp
    for name in ("Hs", "Cs") if env.lstm else ("Hs",):
        S = f[name]
        for t in range(env.T):
            blk = S[env.qoff[t]:env.qoff[t + 1]].view(depth + 1, n[t], Hp)
            src = torch.from_numpy(env.tb["srcH"][t].astype(np.int64)).to(_dev())
            start = torch.where((src >= 0).unsqueeze(1), S[src.clamp(min=0)], torch.zeros(n[t], Hp, device=_dev()))
            assert _same(blk[0], start), (name, t)
            assert bool((blk[0][src < 0] == 0).all()), (name, t)
            assert bool((blk[:, 0] == 0).all()) and bool((blk[:, :, H:] == 0).all()), (name, t)
        assert not bool(torch.isnan(S[:env.Q]).any()), name
    assert not bool(torch.isnan(f["Qs"][:env.R]).any()) and not bool(torch.isnan(f["St"][:, :env.R]).any())
    _guards_intact(env, f)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_forward_only_form_is_bit_identical(case):
    """ggpm_decode_steps_infer (ggpm_level_opts.h_out / c_out on sparse forwards, frozen rows gathered from F_h / F_c
    through srcF): F_h and F_c hold the bits of slot ``depth`` of the training forward's blocks, as the header promises."""
    env = _env(case)
    f, _, _ = _driver(case)
    b = env.infer_buffers()
    assert env.infer(b) == 0
    torch.cuda.synchronize()
    assert _same(b["F_h"][:env.Ftot], _final_rows(env, f["Hs"]))
    assert _all_nan(b["F_h"][env.Ftot:]) and _all_nan(b["Hs"][2 * env.nmax:]) and _all_nan(b["Qs"][2 * env.nmax:])
    if env.lstm:
        assert _same(b["F_c"][:env.Ftot], _final_rows(env, f["Cs"]))
        assert _all_nan(b["F_c"][env.Ftot:]) and _all_nan(b["Cs"][2 * env.nmax:])


_COMPARED = (("Hs", "Cs", "Qs", "St"), ("dF", "dCF", "dX", "DG", "DQ"))


def _assert_same_run(env, a, b, what):
    for side, (x, y) in enumerate(zip(a[:2], b[:2])):
        for k in _COMPARED[side]:
            if x[k] is not None:
                assert _same(x[k], y[k]), (what, k)
    for k in a[2]:
        assert _same(a[2][k], b[2][k]), (what, k)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_driver_is_run_to_run_identical(case):
    """a second driver run on fresh NaN buffers (weights packed once per loop, by its first step): the same bits"""
    env = _env(case)
    _assert_same_run(env, _driver(case), _run_driver(env), "second run")


def _run_unfolded(env):
    """The same sequence step by step through the public calls, as atom_decode issues it with the decode driver off:
    ggpm_gather_rows into a start state -> sparse_forward without gather options; sparse_backward with defer_stash but
    without scatter options -> ggpm_scatter_rows(accumulate = 1).  Every step packs its weights."""
    _lib, lib, F_, _ = _mods()
    P, s, cell = F_._p, F_._stream(), env.cell
    f, b = env.forward_buffers(), env.backward_buffers()
    G, Hp, depth, lstm, ptr = env.G, env.Hp, env.depth, env.lstm, env.ptr
    vp = ctypes.c_void_p
    blocks = []
    for t in range(env.T):
        n, f0, r0, r1, q0, q1 = env.n[t], env.foff[t], env.roff[t], env.roff[t + 1], env.qoff[t], env.qoff[t + 1]
        X = env.X_all[G * f0:G * (f0 + n)].view(G, n, Hp)
        blk = dict(n=n, X=X, Hs=f["Hs"][q0:q1], Cs=f["Cs"][q0:q1] if lstm else None, Qs=f["Qs"][r0:r1], St=f["St"][:, r0:r1])
        blocks.append(blk)
        h_in, c_in = _nan(n, Hp), _nan(n, Hp) if lstm else None
        assert lib.ggpm_gather_rows(P(f["Hs"]), Hp, vp(ptr["srcH", t]), n, Hp, P(h_in), Hp, 0, 0, s) == 0
        if lstm:
            assert lib.ggpm_gather_rows(P(f["Cs"]), Hp, vp(ptr["srcH", t]), n, Hp, P(c_in), Hp, 0, 0, s) == 0
        cell.sparse_forward(rows=n, depth=depth, h_in=h_in, c_in=c_in, frozen=ptr["frozen", t], X=X,
                            pred=(ptr["pred_rowptr", t], ptr["pred_col", t]), Hs=blk["Hs"], Cs=blk["Cs"], Qs=blk["Qs"],
                            St=blk["St"], wpack=f["wpack"], save=True, opts=None, stream=s)
    work = b["work"][:env.work_floats()]
    for t in range(env.T - 1, -1, -1):
        blk, n, f0, r0, q0 = blocks[t], env.n[t], env.foff[t], env.roff[t], env.qoff[t]
        dhin, dcin = _nan(n, Hp), _nan(n, Hp) if lstm else None
        dq = b["DQ"][q0:].data_ptr()
        stash = (b["DG"][0, r0:].data_ptr(), b["DG"][1, r0:].data_ptr()) + \
            ((b["DG"][2, r0:].data_ptr(), dq) if lstm else (dq, None))
        opts = F_.LevelOpts(defer_stash=stash)
        cell.sparse_backward(rows=n, depth=depth, frozen=ptr["frozen", t], Xg=blk["X"][cell.reread],
                             pred=(ptr["pred_rowptr", t], ptr["pred_col", t]), succ=(ptr["succ_rowptr", t], ptr["succ_col", t]),
                             Hs=blk["Hs"], Cs=blk["Cs"], Qs=blk["Qs"], St=blk["St"], d_out=b["dF"][f0:f0 + n],
                             dc_out=b["dCF"][f0:f0 + n] if lstm else None, d_in=dhin, dc_in=dcin,
                             dX=b["dX"][G * f0:G * (f0 + n)].view(G, n, Hp), dW_hidden=b["dW_unused"], ld_dW=env.H, work=work,
                             opts=ctypes.byref(opts), stream=s)
        if lstm:
            assert lib.ggpm_scatter_rows(P(dcin), Hp, vp(ptr["srcF", t]), n, Hp, P(b["dCF"]), Hp, 1, s) == 0
        assert lib.ggpm_scatter_rows(P(dhin), Hp, vp(ptr["srcF", t]), n, Hp, P(b["dF"]), Hp, 1, s) == 0
    wg = env.weight_grads(f, b)
    torch.cuda.synchronize()
    return f, b, wg


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_folded_loop_is_bit_identical_to_public_calls(case):
    """The drivers fold the start-state gather into the step's q^0 / qf^0 launch (gather_*), the scatter-add of dHin / dCin
    into its last backward launch (scatter_*) and pack the weights once (weights_packed).  Both forms copy the same values
    and do the same single fp32 add per element in the same step order, so every state block, the stashes, dX_all,
    dF / dCF, the stacked gate-gradient stashes and the weight gradients contracted from them are the same bits."""
    env = _env(case)
    un = _run_unfolded(env)
    _assert_same_run(env, _driver(case), un, "unfolded")
    for w in un[1]["dW_unused"]:
        assert bool((w == SENTINEL).all())
    _guards_intact(env, *un)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_worker_thread_forms_are_bit_identical(case):
    """*_forward_async -> ggpm_decode_join -> *_backward_async -> join (and infer_async -> join): every join returns 0,
    the results are the synchronous calls' bits, a join with nothing posted returns 0."""
    _lib, lib, _, _ = _mods()
    env = _env(case)
    f, b, i = env.forward_buffers(), env.backward_buffers(), env.infer_buffers()
    assert env.forward(f, fn="ggpm_decode_steps_forward_async") == 0
    assert lib.ggpm_decode_join() == 0
    assert env.backward(f, b, fn="ggpm_decode_steps_backward_async") == 0
    assert lib.ggpm_decode_join() == 0
    assert env.infer(i, fn="ggpm_decode_steps_infer_async") == 0
    assert lib.ggpm_decode_join() == 0
    assert lib.ggpm_decode_join() == 0
    wg = env.weight_grads(f, b)
    torch.cuda.synchronize()
    _assert_same_run(env, _driver(case), (f, b, wg), "worker thread")
    assert _same(i["F_h"][:env.Ftot], _final_rows(env, f["Hs"]))
    _guards_intact(env, f, b, wg)


def _all_untouched(bufs):
    torch.cuda.synchronize()
    for k, v in bufs.items():
        if isinstance(v, torch.Tensor):
            assert _all_nan(v), k
    for w in bufs.get("dW_unused", ()):
        assert bool((w == SENTINEL).all())


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_worker_thread_error_path(case):
    """A descriptor with T = 0 launches nothing: the post returns 0, the next join hands back GGPM_ERR_ARG, the join
    after that 0, every buffer is still NaN."""
    _lib, lib, _, _ = _mods()
    env = _env(case)
    empty, _keep = env.descriptor(0)
    f, b, i = env.forward_buffers(), env.backward_buffers(cotangent=False), env.infer_buffers()
    for post in (lambda: env.forward(f, fn="ggpm_decode_steps_forward_async", desc=empty),
                 lambda: env.backward(f, b, fn="ggpm_decode_steps_backward_async", desc=empty),
                 lambda: env.infer(i, fn="ggpm_decode_steps_infer_async", desc=empty)):
        assert post() == 0
        assert lib.ggpm_decode_join() == _lib.GGPM_ERR_ARG
        assert lib.ggpm_decode_join() == 0
    for bufs in (f, b, i):
        _all_untouched(bufs)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_argument_checks_launch_nothing(case):
    """X_all NULL, Cs_all NULL for an LSTM, bu NULL for a GRU: GGPM_ERR_ARG from every synchronous entry point that takes
    the argument; a work_bytes below the cell's backward workspace: GGPM_ERR_WORKSPACE.  Every buffer is still NaN."""
    _lib, lib, _, _ = _mods()
    env = _env(case)
    f, b, i = env.forward_buffers(), env.backward_buffers(cotangent=False), env.infer_buffers()
    ARG = _lib.GGPM_ERR_ARG
    assert env.forward(f, X=False) == ARG and env.infer(i, X=False) == ARG and env.backward(f, b, X=False) == ARG
    if env.lstm:
        assert env.forward(f, Cs=False) == ARG and env.infer(i, Cs=False) == ARG and env.backward(f, b, Cs=False) == ARG
    else:
        assert env.forward(f, bu=False) == ARG and env.infer(i, bu=False) == ARG
    # one float short of what the LAST step needs: the loop's first level call refuses
    fn = lib.ggpm_lstm_backward_workspace_bytes if env.lstm else lib.ggpm_gru_backward_workspace_bytes
    need = int(fn(env.n[-1], env.H, env.depth))
    assert need <= env.work_floats() * 4
    assert env.backward(f, b, work_bytes=need - 4) == _lib.GGPM_ERR_WORKSPACE
    for bufs in (f, b, i):
        _all_untouched(bufs)
