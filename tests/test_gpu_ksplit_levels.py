"""GPU: the K-split form of q' on column-grouped GRU levels (include/ggpm_hip.h: ggpm_level_opts.q_part).

A column group forms a partial q' over its own K slice of U_r inside kernel A, the next step's gather adds the partials in
group order, and only the last executed step keeps its B launch.  Each case runs the level alone through functional.GruCell's
level calls (the calls rnn.GRU's autograd node makes, with the options struct in the test's hands), with and without the
buffer, and compares every output and gradient with oracle/ref_encoder.py in fp64 under the two bars
tests/test_gpu_level_forms.py applies to the column-grouped forms."""
import ctypes
import time

import numpy as np
import pytest
import torch

import level_form_cases as C
import test_gpu_level_forms as T

pytestmark = pytest.mark.gpu

GUARD = 4096          # floats behind the partial buffer that no launch may touch

# (H, E1, depth, groups): 5 groups with a ragged last group and a partial last row tile; 4, 3 and 2 groups; 4 even groups;
# 5 groups of 8 tiles; and 10 groups, which stay on B launches
CASES = [(300, 40, 3, 5), (300, 817, 2, 4), (300, 1025, 2, 3), (300, 1361, 2, 2), (250, 40, 2, 4), (600, 673, 2, 5),
         (600, 40, 2, 10)]


def _dev():
    return torch.device("cuda:0")


def _nan_buffer(nbytes):
    return torch.full((nbytes // 4 + GUARD,), float("nan"), device=_dev())


def _run(case, mod, xg, bg, w, q_part, save=True):
    """One level call, forward (+ backward) -> (h [E1, Hp], {name: gradient} or None).  ``q_part``: the buffer or None."""
    from ggpm_amd import functional as F_
    E1, H, depth = case.E1, case.H, case.depth
    cell = F_.GruCell(mod.level_params(), C.I, H)
    pred = F_.csr_from_padded(bg, ncols=E1)
    opts = F_.LevelOpts()
    if q_part is not None:
        opts.q_part, opts.q_part_bytes = q_part.data_ptr(), (q_part.numel() - GUARD) * 4
    o = ctypes.byref(opts)
    with torch.no_grad():
        X = torch.empty(3, E1, cell.Hp, device=_dev())
        cell.project_inputs(xg, xg.stride(0), E1, X)
        wpack = cell.alloc_pack()
        Hs, _, Qs, St = cell.alloc_state(E1, depth, save)
        cell.forward(rows=E1, depth=depth, X=X, pred=pred, Hs=Hs, Qs=Qs, St=St, wpack=wpack, save=save, opts=o)
        h = Hs[depth if save else depth & 1]
        if not save:
            return h, None
        dHD = torch.zeros(E1, cell.Hp, device=_dev())
        dHD[:, :H] = w
        dX = torch.empty(3, E1, cell.Hp, device=_dev())
        bufs, hid = cell.dW_buffers()
        work = cell.backward_workspace(E1, depth)
        cell.backward(rows=E1, depth=depth, Xg=X[cell.reread], pred=pred, succ=pred.T, Hs=Hs, Qs=Qs, St=St, d_out=dHD, dX=dX,
                      dW_hidden=hid, work=work, weight_grads=True, opts=o)
        dx = cell.input_grad(dX, xg, E1)
        grads = cell.grads(bufs, hid, cell.input_half_grads(dX, xg, xg.stride(0), E1, bufs))
        torch.cuda.synchronize()
    got = {k: g for (k, _), g in zip(mod.named_parameters(), grads)}
    got["dx"] = dx
    return h, got


def _numpy(case, h, grads):
    return dict({k: v.cpu().numpy() for k, v in grads.items()}, h=h[:, :case.H].cpu().numpy())


@pytest.mark.parametrize("H,E1,depth,groups", CASES, ids=["H%d-E%d-d%d-g%d" % c for c in CASES])
def test_level_on_partial_q_matches_fp64_and_the_b_launch_form(H, E1, depth, groups):
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    t0 = time.perf_counter()
    case = C.Case("GRU", H, E1, depth, None, False, 0)
    form = C.query(case)
    assert form.groups == groups and form.gate_mode == 0 and form.rt2 == 0 and form.fuse_fwd == 0
    lib = _lib.load()
    applies = lib.ggpm_level_ksplit_q(0, E1, H, 0, None)
    assert applies == int(groups <= 5)
    nbytes = int(lib.ggpm_level_q_part_bytes(E1, H))
    assert nbytes == 2 * groups * E1 * form.Hp * 4

    sd = C.weights(case)
    x, bgraph, w = C.dense_inputs(case)
    mod = T._module(case, sd)
    xg, bg, wg = torch.from_numpy(x).to(_dev()), torch.from_numpy(bgraph).to(_dev()), torch.from_numpy(w).to(_dev())

    # training forward + backward on a buffer full of NaN, twice: no NaN comes out, the pad row and the pad columns are zero,
    # nothing behind the buffer is touched, and the two runs agree bit for bit
    runs = []
    for _ in range(2):
        qp = _nan_buffer(nbytes)
        h, grads = _run(case, mod, xg, bg, wg, qp)
        assert bool(torch.isfinite(h).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert float(h[0].abs().max()) == 0.0 and float(h[:, H:].abs().max() if form.Hp > H else 0.0) == 0.0
        assert bool(torch.isnan(qp[nbytes // 4:]).all())
        written = not bool(torch.isnan(qp[:nbytes // 4]).all())
        assert written == bool(applies)          # (10 groups: the B path never looks at the buffer)
        runs.append((h, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k

    # forward only (no stashes, two ping-pong slots): the same h, bit for bit
    h0, _ = _run(case, mod, xg, bg, wg, _nan_buffer(nbytes), save=False)
    assert torch.equal(h0, runs[0][0])

    # without a buffer: the B launches
    hb, gradsb = _run(case, mod, xg, bg, wg, None)
    if not applies:
        assert torch.equal(hb, runs[0][0])
        for k in gradsb:
            assert torch.equal(gradsb[k], runs[0][1][k]), k

    # both forms under the oracle's bars (every gradient: Qs is what the backward needs)
    want64 = T._dense_oracle(case, sd, x, bgraph, w, torch.float64)
    want32 = T._dense_oracle(case, sd, x, bgraph, w, torch.float32)
    T._check(case, form, _numpy(case, *runs[0]), want64, want32, t0)
    T._check(case, form, _numpy(case, hb, gradsb), want64, want32, t0)


def test_too_small_a_buffer_is_refused():
    """a q_part below ggpm_level_q_part_bytes: the workspace error, nothing launched"""
    from ggpm_amd import _lib
    case = C.Case("GRU", 300, 40, 2, None, False, 0)
    x, bgraph, w = C.dense_inputs(case)
    mod = T._module(case, C.weights(case))
    xg, bg, wg = torch.from_numpy(x).to(_dev()), torch.from_numpy(bgraph).to(_dev()), torch.from_numpy(w).to(_dev())
    nbytes = int(_lib.load().ggpm_level_q_part_bytes(case.E1, case.H))
    qp = _nan_buffer(nbytes)
    short = qp[:nbytes // 4 - 1 + GUARD]          # _run reports numel - GUARD floats
    with pytest.raises(RuntimeError, match=r"\(code 4\)"):
        _run(case, mod, xg, bg, wg, short)
    assert bool(torch.isnan(qp).all())
