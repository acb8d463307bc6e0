"""GPU: the forms a GRU / LSTM level call takes only through ``ggpm_level_opts.gate_dtype`` and ``prefer_narrow``
(tests/level_form_cases.py: OPT_DENSE, OPT_SPARSE), each against a high-precision reference of the same arithmetic.

Each case first asserts with ggpm_level_form_query, under the case's options, that the call takes the form the table
states (st16 included).  How the call is made: a dense case without prefer_narrow sets ``gate_dtype`` on rnn.GRU / rnn.LSTM;
prefer_narrow and the sparse gate dtypes have no Python attribute and go through the cell adapters of
ggpm_amd/functional.py with ``opts=``, from NaN-filled, guarded buffers (tests/level_form_checks.py).  By arithmetic class:

* fp32 arithmetic (gate modes 0 and 2, one or two row tiles): the two bars of tests/test_gpu_level_forms.py against the fp64
  oracle; a prefer_narrow case also holds ``h`` within 5e-6 (norm-wise, include/ggpm_hip.h) of the default call.
* bf16 operands (gate mode 1): the row-wise criteria of test_bf16_level_kernels_match_the_bf16_oracle against
  oracle/ref_encoder.py rounding the same operands at the same points -- "bf16" / "bf16w" by whether the level's shortest
  weight-gradient contraction takes the bf16 tall kernel, "bf16s" under bf16 storage; sparse cases against
  gru_sparse_forward / lstm_sparse_forward with ``gate_dtype``.
* forward-only: the call without stashes returns ``h`` (LSTM: and ``c``) bit-identical to the training forward out of the
  two ping-pong slots -- under bf16 storage through ggpm_level_opts.h_out, which keeps the storage.

profiles/level_option_forms.txt records the distances each case printed."""
import time

import numpy as np
import pytest
import torch

import level_form_cases as C
import level_form_checks as K
from golden_utils import rel_err

pytestmark = pytest.mark.gpu

NARROW_TOL = 5e-6      # include/ggpm_hip.h, ggpm_level_opts.prefer_narrow: agreement with the default form, norm-wise


def _stated_form(case):
    form = C.query(case)
    assert form is not None and C.reduced_opt(form) == case.form, (form and C.reduced_opt(form), case.form)
    return form


def _dense_by_module(case, sd, x, bgraph, w, gate_dtype):
    """forward + backward through rnn.GRU / rnn.LSTM with the ``gate_dtype`` attribute -> (results, (h, c or None))"""
    mod = K.module(case, sd)
    mod.gate_dtype = gate_dtype
    xg = torch.from_numpy(x).to(K.dev()).requires_grad_(True)
    out = mod(xg, torch.from_numpy(bgraph).to(K.dev()))
    h, c = (out, None) if case.cell == "GRU" else out
    (h * torch.from_numpy(w).to(K.dev())).sum().backward()
    got = dict({k: v.grad.cpu().numpy() for k, v in mod.named_parameters()}, h=h.detach().cpu().numpy(),
               dx=xg.grad.cpu().numpy())
    return got, (h.detach(), None if c is None else c.detach())


def _dense_hip(case, sd, x, bgraph, w, gate_dtype, prefer_narrow):
    if prefer_narrow:
        opts = C.level_opts(case._replace(gate_dtype=gate_dtype, prefer_narrow=1))
        return K.dense_by_adapters(case, K.module(case, sd), x, bgraph, w, opts)
    return _dense_by_module(case, sd, x, bgraph, w, gate_dtype)


def _dense_forward_only(case, form, sd, x, bgraph):
    """-> (h, c or None) [E1, >= H] of the call without stashes, out of two ping-pong slots"""
    if form.st16:      # the forward-only form that keeps bf16 storage: ggpm_level_opts.h_out
        return K.dense_by_adapters(case, K.module(case, sd), x, bgraph, None, C.level_opts(case), train=False, h_out=True)
    if case.prefer_narrow:
        return K.dense_by_adapters(case, K.module(case, sd), x, bgraph, None, C.level_opts(case), train=False)
    # (as tests/test_gpu_level_forms.py: a module with frozen parameters and a detached input keeps no stashes)
    frozen = K.module(case, sd).requires_grad_(False)
    frozen.gate_dtype = case.gate_dtype
    with torch.no_grad():
        out = frozen(torch.from_numpy(x).to(K.dev()), torch.from_numpy(bgraph).to(K.dev()))
    out = (out, None) if case.cell == "GRU" else out
    for t in out:
        assert t is None or (not t.requires_grad and t.untyped_storage().nbytes() == 2 * case.E1 * form.Hp * 4)
    return out


def _assert_same_state(case, train, infer):
    for name, a, b in zip("hc", train, infer):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a[:, :case.H], b[:, :case.H]), "forward-only %s differs from the training forward" % name


def _bf16_rows_of_sparse(case, submess, bgraph):
    """The rows of a sparse call that say something about its arithmetic: the state rows it recomputes (a frozen row's
    state is a copy) and, of the incoming-state gradient, the frozen rows a recomputed row reads (a recomputed row's is
    zero, and a frozen row nobody reads gets its cotangent back unchanged)."""
    sub = np.sort(submess)
    read = np.setdiff1d(np.unique(bgraph[bgraph > 0]), sub) - 1      # (dh_in, dc_in: row 0, the pad row, is cut off)
    assert len(read) >= len(sub) // 2
    rows = [("h", "h", sub), ("dx", "dx", None), ("dh_in", "dx", read)]
    return rows + ([("c", "h", sub), ("dc_in", "dx", read)] if case.cell == "LSTM" else [])


@pytest.mark.parametrize("case", C.OPT_DENSE, ids=C.case_id)
def test_dense_level_of_every_option_form(case):
    """forward + backward of a dense level on every form only options reach at H = 250 / 300 / 600, and the same level
    forward-only"""
    from ggpm_amd import _lib
    t0 = time.perf_counter()
    form = _stated_form(case)
    sd = C.weights(case)
    x, bgraph, w = C.dense_inputs(case)
    got, state = _dense_hip(case, sd, x, bgraph, w, case.gate_dtype, case.prefer_narrow)
    assert (got["h"][0] == 0).all()
    _assert_same_state(case, state, _dense_forward_only(case, form, sd, x, bgraph))
    if form.gate_mode == 1:
        lib = _lib.load(build_if_missing=False)
        assert bool(lib.ggpm_level_bf16_storage(case.E1, case.H)) == bool(form.st16)
        mode = K.bf16_oracle_mode(lib, case.H, (case.depth - 1) * case.E1, form.st16)
        got32, _ = _dense_hip(case, sd, x, bgraph, w, 0, 0)
        want = K.dense_oracle(case, sd, x, bgraph, w, torch.float32, gate_dtype=mode)
        K.check_bf16_level("%s form %s %.2f s" % (C.case_id(case), case.form, time.perf_counter() - t0), got, got32, want,
                           mode, list(sd))
        return
    if case.prefer_narrow:
        base, _ = _dense_hip(case, sd, x, bgraph, w, case.gate_dtype, 0)
        narrow = rel_err(got["h"], base["h"])
        print("level form %-26s two row tiles against the default form: h %.2e" % (C.case_id(case), narrow))
        assert narrow <= NARROW_TOL, narrow
    K.check(case, form, got, K.dense_oracle(case, sd, x, bgraph, w, torch.float64),
            K.dense_oracle(case, sd, x, bgraph, w, torch.float32), t0)


@pytest.mark.parametrize("case", C.OPT_SPARSE, ids=C.case_id)
def test_sparse_level_of_every_option_form_of_the_tested_classes(case):
    """sparse forward + backward with a quarter of the rows recomputed under gate_dtype 1 (bf16 operands) and 3 (split
    operands) on tg 4 / 5, two groups and one group, and the same call forward-only"""
    from ggpm_amd import _lib
    t0 = time.perf_counter()
    form = _stated_form(case)
    sd = C.weights(case)
    inputs = C.sparse_case_inputs(case)
    mod = K.module(case, sd)
    got, state = K.sparse_by_adapters(case, mod, inputs, C.level_opts(case))
    _assert_same_state(case, state, K.sparse_by_adapters(case, mod, inputs, C.level_opts(case), train=False))
    frozen_rows = np.setdiff1d(np.arange(case.E1), inputs[2])
    assert np.array_equal(got["h"][frozen_rows], inputs[0][frozen_rows])        # a frozen row keeps its state, bit for bit
    if form.gate_mode == 1:
        lib = _lib.load(build_if_missing=False)
        mode = K.bf16_oracle_mode(lib, case.H, case.depth * case.E1, False)      # (a sparse level contracts dq^0 as well)
        got32, _ = K.sparse_by_adapters(case, mod, inputs, None)
        want = K.sparse_oracle(case, sd, inputs, torch.float32, gate_dtype=mode)
        K.check_bf16_level("%s form %s %.2f s" % (C.case_id(case), case.form, time.perf_counter() - t0), got, got32, want,
                           mode, list(sd), rows=_bf16_rows_of_sparse(case, inputs[2], inputs[4]))
        return
    K.check(case, form, got, K.sparse_oracle(case, sd, inputs, torch.float64),
            K.sparse_oracle(case, sd, inputs, torch.float32), t0)
