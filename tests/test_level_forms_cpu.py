"""CPU: ggpm_level_form_query (host only) against the case table of tests/level_form_cases.py -- every form a level call
can take at the configured hidden sizes has a case that tests/test_gpu_level_forms.py runs against fp64, no form asks for
more LDS than a workgroup has, and the accepted hidden sizes are the documented ones."""
import itertools

import pytest

import level_form_cases as C
from ggpm_amd import functional as F_

LDS_BYTES = 160 * 1024          # MI355X LDS per workgroup: what the dispatch budgets against


def _table(cases):
    forms = {}
    for c in cases:
        forms.setdefault((c.cell, c.H), set()).add(c.form)
    return forms


def test_every_case_takes_the_form_the_table_states():
    for c in C.DENSE + C.SPARSE + C.LIMIT_DENSE + C.LIMIT_SPARSE:
        f = C.query(c)
        assert f is not None and C.reduced(f) == c.form, (C.case_id(c), f and C.reduced(f), c.form)


def test_the_table_keeps_the_cases_the_lattice_alone_does_not_ask_for():
    """The coverage tests hold every form to SOME case; these are named on top of that: the upper end (last row tile full)
    of the two-group classes, depth 3 on the H = 600 two-group class (two full gate-product steps with two tiles per
    wave), the natural two-row-tile GRU level, the three sparse classes, and the cases at the accepted limits."""
    dense = {(c.cell, c.H, c.E1): c for c in C.DENSE}
    assert len(dense) == len(C.DENSE)
    for cell in ("GRU", "LSTM"):
        for H, cls in ((250, (8, 2)), (300, (10, 2)), (600, (19, 2))):
            lo, hi = dense[cell, H, 1361], dense[cell, H, 2048]
            assert lo.form[:2] == hi.form[:2] == cls and hi.E1 % 16 == 0
            assert C.reduced(C.query(hi._replace(E1=hi.E1 + 1)))[:2] != cls        # 2048 is the class's last E1
            assert lo.depth == hi.depth == (3 if H == 600 else 2), (cell, H, lo.depth, hi.depth)
        for H in C.HIDDEN:
            assert dense[cell, H, 40].depth >= 2 and dense[cell, H, 2049].form[1] == 1
    assert dense["GRU", 300, 8177].form == (19, 1, 0, 1, 0, 0)
    assert all(c.depth >= 2 and not c.sparse for c in C.DENSE + C.LIMIT_DENSE)
    sparse = {(c.cell, c.H, c.E1): c for c in C.SPARSE}
    assert sorted(sparse) == sorted((cell, H, E1) for cell in ("GRU", "LSTM") for H in C.HIDDEN for E1 in C.SPARSE_E1)
    assert all(c.sparse and c.depth >= 2 and abs(4 * c.ms - c.E1) < 4 for c in C.SPARSE + C.LIMIT_SPARSE)
    assert sorted((c.cell, c.H, c.E1) for c in C.LIMIT_DENSE) == sorted(
        [("GRU", 1264, E1) for E1 in (40, 673, 1361, 2049)] + [("GRU", 840, 2049), ("GRU", 850, 2049)]
        + [("LSTM", 848, E1) for E1 in (40, 1025, 2049)])
    assert [(c.cell, c.H, c.E1) for c in C.LIMIT_SPARSE] == [("LSTM", 848, 450)]


def test_every_reachable_dense_form_has_a_case():
    """cell x H in {250, 300, 600} x E1 = 2 .. 4096, dense training call, default options"""
    table = _table(C.DENSE)
    for cell, H in itertools.product(("GRU", "LSTM"), C.HIDDEN):
        for E1 in range(2, 4097):
            form = C.reduced(F_.level_form(cell == "LSTM", E1, H))
            assert form in table[cell, H], "no dense case covers (cell, H, E1, form) = %r" % ((cell, H, E1, form),)


def test_every_sparse_form_of_the_tested_classes_has_a_case():
    """... and sparse calls, over the E1 of the three (tg, groups) classes the sparse cases stand in"""
    table = _table(C.SPARSE)
    for cell, H in itertools.product(("GRU", "LSTM"), C.HIDDEN):
        classes = {C.reduced(F_.level_form(cell == "LSTM", E1, H, sparse=True))[:2] for E1 in C.SPARSE_E1}
        assert len(classes) == 3, (cell, H, classes)
        for E1 in range(2, 4097):
            form = C.reduced(F_.level_form(cell == "LSTM", E1, H, sparse=True))
            if form[:2] in classes:
                assert form in table[cell, H], "no sparse case covers (cell, H, E1, form) = %r" % ((cell, H, E1, form),)


# ---- the forms only options reach (C.OPT_DENSE, C.OPT_SPARSE; tests/test_gpu_level_option_forms.py runs them)
SWEEP_E1 = tuple(range(2, 4097)) + (6143, 6144, 6145, 8177, 8192, 8193, 12289)
SWEEP_OPTS = tuple((dt, pn) for dt in range(4) for pn in (0, 1))


def _with_st16(c):
    """a case's form as reduced_opt states it (a default case never stores bf16)"""
    return c.form if len(c.form) == 7 else c.form + (0,)


def _table_opt(cases):
    forms = {}
    for c in cases:
        forms.setdefault((c.cell, c.H), set()).add(_with_st16(c))
    return forms


def _forward_form(form7):
    """a reduced_opt form without fuse_bwd: what a forward call can tell apart"""
    return form7[:5] + form7[6:]


def _sweep(sparse, training=True, h_out=False):
    """-> (cell, H, E1, gate_dtype, prefer_narrow, reduced_opt form) over the option sweep"""
    import ctypes
    for cell, H, (dt, pn) in itertools.product(("GRU", "LSTM"), C.HIDDEN, SWEEP_OPTS):
        o = F_.LevelOpts(gate_dtype=dt, prefer_narrow=pn)
        if h_out:
            o.h_out = ctypes.c_void_p(256)      # host only: an address that is never read
        for E1 in SWEEP_E1:
            yield cell, H, E1, dt, pn, C.reduced_opt(F_.level_form(cell == "LSTM", E1, H, sparse=sparse, training=training,
                                                                   opts=o))


def _sparse_classes():
    return {(cell, H): {C.reduced(F_.level_form(cell == "LSTM", E1, H, sparse=True))[:2] for E1 in C.SPARSE_E1}
            for cell, H in itertools.product(("GRU", "LSTM"), C.HIDDEN)}


def test_every_option_case_takes_the_form_the_table_states():
    """... including st16, under the case's own gate_dtype / prefer_narrow; and the table is minimal: no two option cases
    state the same form, none states a form a default case already holds, so deleting any one of them leaves its form
    without a case and fails one of the coverage tests below."""
    seen = {(c.cell, c.H, c.sparse, _with_st16(c)) for c in C.DENSE + C.SPARSE}
    for c in C.OPT_DENSE + C.OPT_SPARSE:
        f = C.query(c)
        assert f is not None and len(c.form) == 7 and C.reduced_opt(f) == c.form, (C.case_id(c), f and C.reduced_opt(f), c.form)
        assert c.gate_dtype or c.prefer_narrow, C.case_id(c)
        key = (c.cell, c.H, c.sparse, c.form)
        assert key not in seen, "two cases for one form: %s" % C.case_id(c)
        seen.add(key)
    ids = [C.case_id(c) for c in C.DENSE + C.SPARSE + C.OPT_DENSE + C.OPT_SPARSE]
    assert len(set(ids)) == len(ids)
    assert all(not c.sparse and c.depth == (3 if (c.H, c.form[:2]) == (600, (19, 2)) else 2) for c in C.OPT_DENSE)
    assert all(c.sparse and c.E1 in C.SPARSE_E1 and abs(4 * c.ms - c.E1) < 4 and not c.prefer_narrow for c in C.OPT_SPARSE)


def test_every_option_case_sits_at_the_lower_end_of_its_class():
    """the smallest E1 of the sweep that takes the form under the case's options; 40 for the first class"""
    for c in C.OPT_DENSE:
        o = C.level_opts(c)
        first = next(E1 for E1 in SWEEP_E1 if C.reduced_opt(F_.level_form(c.cell == "LSTM", E1, c.H, opts=o)) == c.form)
        assert c.E1 == (40 if first == 2 else first), (C.case_id(c), first)


def test_every_dense_form_the_options_reach_has_a_case():
    """cell x H in {250, 300, 600} x E1 = 2 .. 4096 and the sizes around bf16 storage and the natural two row tiles x
    gate_dtype 0 .. 3 x prefer_narrow 0 / 1, dense training call"""
    table = _table_opt(C.DENSE + C.OPT_DENSE)
    reached = set()
    for cell, H, E1, dt, pn, form in _sweep(sparse=False):
        assert form in table[cell, H], "no dense case covers (cell, H, E1, gate_dtype, prefer_narrow, form) = %r" % (
            (cell, H, E1, dt, pn, form),)
        reached.add((cell, H, form))
    # ... and the lattice reaches every case of the table: 73 + 38 forms only options reach
    assert {(c.cell, c.H, c.form) for c in C.OPT_DENSE} <= reached
    # (two more GRU cases: the two-row-tile single groups a DEFAULT call takes from 8177 rows at H = 250 / 600 -- DENSE
    # holds the one of H = 300 -- stand in OPT_DENSE at 2049 rows through prefer_narrow)
    extra = [c for c in C.OPT_DENSE if c.cell == "GRU" and c.form in ((16, 1, 0, 1, 0, 0, 0), (38, 1, 0, 1, 0, 0, 0))]
    assert sorted((c.H, c.E1, c.prefer_narrow) for c in extra) == [(250, 2049, 1), (600, 2049, 1)]
    assert [sum(c.cell == cell for c in C.OPT_DENSE if c not in extra) for cell in ("GRU", "LSTM")] == [73, 38]


def test_every_sparse_form_the_options_reach_in_the_tested_classes_has_a_case():
    """the same sweep for sparse calls, over the three (tg, groups) classes the sparse cases stand in: 33 forms"""
    table, classes = _table_opt(C.SPARSE + C.OPT_SPARSE), _sparse_classes()
    reached = set()
    for cell, H, E1, dt, pn, form in _sweep(sparse=True):
        if form[:2] in classes[cell, H]:
            assert form in table[cell, H], "no sparse case covers (cell, H, E1, gate_dtype, prefer_narrow, form) = %r" % (
                (cell, H, E1, dt, pn, form),)
            reached.add((cell, H, form))
    assert {(c.cell, c.H, c.form) for c in C.OPT_SPARSE} <= reached and len(C.OPT_SPARSE) == 33


@pytest.mark.parametrize("sparse", [False, True])
def test_a_forward_only_call_takes_no_forward_form_of_its_own(sparse):
    """training = 0, with and without ggpm_level_opts.h_out (which keeps bf16 storage): every forward form -- the form
    without fuse_bwd -- is the forward form of a training case, so the GPU tests check forward-only calls by bit
    equality with the training forward alone."""
    cases = C.SPARSE + C.OPT_SPARSE if sparse else C.DENSE + C.OPT_DENSE
    table = {k: {_forward_form(f) for f in v} for k, v in _table_opt(cases).items()}
    classes = _sparse_classes()
    for h_out in (False, True):
        for cell, H, E1, dt, pn, form in _sweep(sparse=sparse, training=False, h_out=h_out):
            assert form[5] == 0        # no backward, nothing fused into it
            if sparse and form[:2] not in classes[cell, H]:
                continue
            assert _forward_form(form) in table[cell, H], \
                "a forward-only form without a training case: %r" % ((cell, H, E1, dt, pn, h_out, form),)


def _accepted_hp(lstm):
    return [hp for hp in range(16, 2049, 16) if F_.level_form(lstm, 40, hp) is not None]


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_no_form_exceeds_the_lds_of_a_workgroup(cell):
    """Every accepted Hp x the lower end of every group count x sparse x training x gate dtype x prefer_narrow: each
    launch's dynamic LDS fits, and the geometry is consistent (groups = ceil(tiles / tg), a non-empty last group)."""
    lstm = cell == "LSTM"
    hps = _accepted_hp(lstm)
    assert hps == list(range(16, (C.LSTM_MAX_H if lstm else C.GRU_MAX_H) + 1, 16))
    rows = sorted({2} | {16 * (256 // g) + 1 for g in range(1, 65)})
    opts = [F_.LevelOpts(gate_dtype=dt, prefer_narrow=pn) for dt in range(4) for pn in (0, 1)]
    for hp, E1, o, sparse, training in itertools.product(hps, rows, opts, (False, True), (False, True)):
        f = F_.level_form(lstm, E1, hp, sparse=sparse, training=training, opts=o)
        what = (cell, hp, E1, o.gate_dtype, o.prefer_narrow, sparse, training)
        assert f is not None, what
        assert max(f.lds_fwd_a, f.lds_fwd_b, f.lds_bwd_a, f.lds_bwd_b) <= LDS_BYTES, \
            (what, f.lds_fwd_a, f.lds_fwd_b, f.lds_bwd_a, f.lds_bwd_b)
        assert f.Hp == hp and f.tiles * 16 == hp and 1 <= f.tg <= f.tiles, (what, f.tiles, f.tg)
        assert f.groups == -(-f.tiles // f.tg) and 0 < f.tiles - (f.groups - 1) * f.tg <= f.tg, (what, f.tiles, f.tg, f.groups)
        assert f.lds_fwd_a > 0 and (f.lds_fwd_b > 0) == (sparse or not f.fuse_fwd), what
        if training:
            assert f.lds_bwd_a > 0 and (f.lds_bwd_b > 0) == (not f.fuse_bwd), what
        else:
            assert (f.fuse_bwd, f.lds_bwd_a, f.lds_bwd_b) == (0, 0, 0), what


@pytest.mark.parametrize("H", [250, 300, 600])
def test_backward_workspace_layout_is_the_documented_one(H):
    """Where a backward leaves its gate stashes inside `work`, and how large `work` is: packed transposes first (3 GRU /
    4 LSTM slots of the largest gate mode's size), then the stashes of `depth` slots each, the dq stash, six scratch slots,
    for the GRU 256 * Hp floats of column-sum scratch, and the split-K workspace.  Host-only entry points: `work` is an
    address that is never read."""
    import ctypes
    from ggpm_amd import _lib
    lib = _lib.load()
    Hp = int(lib.ggpm_padded_hidden(H))
    slotW_gru, rem = divmod(int(lib.ggpm_gru_pack_floats(H)) - Hp, 3)
    slotW_lstm, rem4 = divmod(int(lib.ggpm_lstm_pack_floats(H)), 4)
    assert rem == 0 and rem4 == 0
    work = 1 << 20
    for E1, depth in itertools.product((2, 40, 2049), (1, 2, 20)):
        slot = E1 * Hp
        gemm_ws = int(lib.ggpm_gemm_workspace_bytes(H, H, depth * E1))
        p = [ctypes.c_void_p() for _ in range(3)]
        assert lib.ggpm_gru_backward_stashes(work, E1, H, depth, ctypes.byref(p[0]), ctypes.byref(p[1])) == _lib.GGPM_OK
        assert p[0].value == work + 4 * 3 * slotW_gru, (E1, depth)
        assert p[1].value == p[0].value + 4 * depth * slot, (E1, depth)
        assert lib.ggpm_lstm_backward_stashes(work, E1, H, depth, *(ctypes.byref(x) for x in p)) == _lib.GGPM_OK
        assert p[0].value == work + 4 * 4 * slotW_lstm, (E1, depth)
        assert p[1].value == p[0].value + 4 * depth * slot and p[2].value == p[1].value + 4 * depth * slot, (E1, depth)
        assert int(lib.ggpm_gru_backward_workspace_bytes(E1, H, depth)) == \
            4 * (3 * depth * slot + 6 * slot + 3 * slotW_gru + 256 * Hp) + gemm_ws + 256, (E1, depth)
        assert int(lib.ggpm_lstm_backward_workspace_bytes(E1, H, depth)) == \
            4 * (4 * depth * slot + 6 * slot + 4 * slotW_lstm) + gemm_ws + 256, (E1, depth)


def test_accepted_hidden_sizes_are_the_documented_ones():
    """include/ggpm_hip.h, "Accepted hidden sizes": GRU H <= 1264, LSTM H <= 848; beyond: GGPM_ERR_UNSUPPORTED"""
    import ctypes
    from ggpm_amd import _lib
    lib, out = _lib.load(), F_.LevelForm()
    ok, bad_arg, refused = _lib.GGPM_OK, _lib.GGPM_ERR_ARG, _lib.GGPM_ERR_UNSUPPORTED
    for lstm, H, want in ((0, C.GRU_MAX_H, ok), (0, C.GRU_MAX_H + 1, refused), (1, C.LSTM_MAX_H, ok),
                          (1, C.LSTM_MAX_H + 1, refused)):
        for sparse, training, E1 in itertools.product((0, 1), (0, 1), (2, 40, 2049)):
            assert lib.ggpm_level_form_query(lstm, E1, H, sparse, training, None, ctypes.byref(out)) == want, (lstm, H, E1)
    assert lib.ggpm_level_form_query(0, 0, 300, 0, 1, None, ctypes.byref(out)) == bad_arg
    assert lib.ggpm_level_form_query(0, 40, 0, 0, 1, None, ctypes.byref(out)) == bad_arg
    assert lib.ggpm_level_form_query(1, 40, 300, 0, 1, None, None) == bad_arg
    # the LSTM's second limit: 32-bit byte offsets inside a slot
    edge = -(-(1 << 30) // 304)          # the first E1 with E1 * Hp >= 2^30 at H = 300
    assert F_.level_form(True, edge, 300) is None and F_.level_form(True, edge - 1, 300) is not None
    # the fused single-group GRU forward ends between Hp = 848 and Hp = 864
    assert F_.level_form(False, 2049, 840).fuse_fwd == 1 and F_.level_form(False, 2049, 850).fuse_fwd == 0
