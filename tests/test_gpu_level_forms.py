"""GPU: every form a GRU / LSTM level call can take (tests/level_form_cases.py) against the fp64 oracle, and the accepted
hidden-size limits.

Each case first asserts with ggpm_level_form_query that the call takes the form the table states, then compares every
output and gradient with oracle/ref_encoder.py in fp64 under two bars: the project's 1e-4 (BASELINE.json), and at most
3x (+1e-6) the distance of the oracle's own fp32 CPU run from fp64 -- the margin
test_gate_products_on_split_operands_keep_fp32_accuracy grants split operands over fp32 MFMA.  profiles/level_forms.txt
records the distances each case printed."""
import time

import pytest
import torch

import level_form_cases as C
# (the comparison helpers are shared with tests/test_gpu_level_option_forms.py; TOL and the two bars live with them)
from level_form_checks import TOL, check as _check, dense_oracle as _dense_oracle, dev as _dev, module as _module, \
    sparse_oracle as _sparse_oracle  # noqa: F401

pytestmark = pytest.mark.gpu


def _dense_hip(case, sd, x, bgraph, w):
    """-> (outputs and gradients of forward + backward, the module and its device inputs for further calls)"""
    mod = _module(case, sd)
    xg = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    bg = torch.from_numpy(bgraph).to(_dev())
    out = mod(xg, bg)
    h = out if case.cell == "GRU" else out[0]
    (h * torch.from_numpy(w).to(_dev())).sum().backward()
    got = dict({k: v.grad.cpu().numpy() for k, v in mod.named_parameters()}, h=h.detach().cpu().numpy(),
               dx=xg.grad.cpu().numpy())
    return got, out, mod, xg, bg


def _run_dense(case):
    t0 = time.perf_counter()
    form = C.query(case)
    assert form is not None and C.reduced(form) == case.form, (C.reduced(form), case.form)
    sd = C.weights(case)
    x, bgraph, w = C.dense_inputs(case)
    got, out, mod, xg, bg = _dense_hip(case, sd, x, bgraph, w)
    assert (got["h"][0] == 0).all()
    # The same forward without stashes (the STASH = false kernel instantiations, the result in the two-slot ping-pong):
    # bit-identical h, and c.  The level keeps its stashes whenever an input or a parameter requires a gradient, whatever
    # the grad mode, so this call goes to a module with frozen parameters and a detached input.
    frozen = _module(case, sd).requires_grad_(False)
    with torch.no_grad():
        out0 = frozen(xg.detach(), bg)
    for a, b in zip((out,) if case.cell == "GRU" else out, (out0,) if case.cell == "GRU" else out0):
        # (a view of the two ping-pong slots, not of the training forward's depth + 1)
        assert not b.requires_grad and b.untyped_storage().nbytes() == 2 * case.E1 * form.Hp * 4
        assert torch.equal(a.detach(), b)
    _check(case, form, got, _dense_oracle(case, sd, x, bgraph, w, torch.float64),
           _dense_oracle(case, sd, x, bgraph, w, torch.float32), t0)


@pytest.mark.parametrize("case", C.DENSE, ids=C.case_id)
def test_dense_level_of_every_form_matches_fp64(case):
    """rnn.GRU / rnn.LSTM forward + backward on every form of the lattice at H = 250 / 300 / 600"""
    _run_dense(case)


@pytest.mark.parametrize("case", C.LIMIT_DENSE, ids=C.case_id)
def test_dense_level_at_the_accepted_hidden_sizes_matches_fp64(case):
    """... and at the largest hidden sizes the entry points accept (up to five tiles per wave; every launch within a few
    hundred bytes of the LDS), and on both sides of the last fused single-group GRU forward"""
    _run_dense(case)


def _run_sparse(case):
    t0 = time.perf_counter()
    form = C.query(case)
    assert form is not None and C.reduced(form) == case.form, (C.reduced(form), case.form)
    sd = C.weights(case)
    inputs = C.sparse_case_inputs(case)
    h, c, submess, x, bg, coef = inputs
    mod = _module(case, sd)
    ht, ct = (torch.from_numpy(a).to(_dev()).requires_grad_(True) for a in (h, c))
    # the inputs arrive as the decoder hands them over: a column slice of a padded [ms, ceil4(I)] buffer
    xbuf = torch.zeros(case.ms, (C.I + 3) // 4 * 4, device=_dev())
    xbuf[:, :C.I] = torch.from_numpy(x).to(_dev())
    xleaf = xbuf.requires_grad_(True)
    xt = xleaf[:, :C.I]
    sm, bgt, cf = (torch.from_numpy(a).to(_dev()) for a in (submess, bg, coef))
    if case.cell == "GRU":
        ho = mod.sparse_forward(ht, xt, sm, bgt)
        (cf[0] * ho).sum().backward()
        got = {}
    else:
        ho, co = mod.sparse_forward((ht, ct), xt, sm, bgt)
        ((cf[0] * ho).sum() + (cf[1] * co).sum()).backward()
        got = {"c": co.detach().cpu().numpy(), "dc_in": ct.grad.cpu().numpy()[1:]}
    got.update({k: v.grad.cpu().numpy() for k, v in mod.named_parameters()}, h=ho.detach().cpu().numpy(),
               dh_in=ht.grad.cpu().numpy()[1:], dx=xleaf.grad[:, :C.I].cpu().numpy())
    assert float(xleaf.grad[:, C.I:].abs().sum()) == 0.0
    _check(case, form, got, _sparse_oracle(case, sd, inputs, torch.float64), _sparse_oracle(case, sd, inputs, torch.float32),
           t0)


@pytest.mark.parametrize("case", C.SPARSE + C.LIMIT_SPARSE, ids=C.case_id)
def test_sparse_level_of_every_tested_class_matches_fp64(case):
    """sparse_forward with a quarter of the rows recomputed: new state, gradients of the incoming state, the inputs and
    every parameter, on tg 4 / 5, two groups and one group (the full-level form of the decode steps), and at the
    LSTM's largest hidden size"""
    _run_sparse(case)


@pytest.mark.parametrize("cell,H", [("GRU", C.GRU_MAX_H + 1), ("LSTM", C.LSTM_MAX_H + 1)])
def test_hidden_sizes_past_the_limit_are_refused_and_leave_nothing_behind(cell, H):
    """One past the accepted hidden size: forward and sparse_forward raise the library's "not supported" error, and a
    small level on the same stream afterwards still matches its oracle (no stale error, no half-issued launch)."""
    big = C.Case(cell, H, 40, 2, None, False, 10)
    assert C.query(big) is None
    sd = C.weights(big)
    x, bgraph, _ = C.dense_inputs(big)
    mod = _module(big, sd)
    with pytest.raises(RuntimeError, match=r"not supported.*\(code 3\)"):
        mod(torch.from_numpy(x).to(_dev()).requires_grad_(True), torch.from_numpy(bgraph).to(_dev()))
    h, c, submess, xs, bg, _ = C.sparse_case_inputs(big)
    ht, ct, xt, sm, bgt = (torch.from_numpy(a).to(_dev()) for a in (h, c, xs, submess, bg))
    with pytest.raises(RuntimeError, match=r"not supported.*\(code 3\)"):
        mod.sparse_forward(ht.requires_grad_(True) if cell == "GRU" else (ht.requires_grad_(True), ct), xt, sm, bgt)
    _run_dense(next(c for c in C.DENSE if (c.cell, c.H, c.E1) == (cell, 300, 40)))
