"""Host side of the K-split form of q' (include/ggpm_hip.h: ggpm_level_opts.q_part): which level calls take it, the size of
the buffer, and that neither the form query nor the other sizes move.  No GPU: every entry point called here is host only."""
import ctypes

import pytest

from ggpm_amd import _lib
from ggpm_amd import functional as F_
from ggpm_amd.fused import EncDims

HIDDEN = (250, 300, 600)
MAX_GROUPS = 5
FORM_FIELDS = [f for f, _ in F_.LevelForm._fields_]


def _ksplit(lstm, E1, H, sparse=False, opts=None):
    return _lib.load().ggpm_level_ksplit_q(int(lstm), E1, H, int(sparse), None if opts is None else ctypes.byref(opts))


def _form_tuple(form):
    return None if form is None else tuple(getattr(form, f) for f in FORM_FIELDS)


@pytest.mark.parametrize("H", HIDDEN)
def test_q_part_size_is_two_blocks_of_one_partial_row_set_per_group(H):
    lib = _lib.load()
    Hp = F_.padded_hidden(H)
    for E1 in (2, 40, 401, 673, 817, 1025, 1361, 2048, 2049, 4096):
        form = F_.level_form(False, E1, H, training=True)
        assert int(lib.ggpm_level_q_part_bytes(E1, H)) == 2 * form.groups * E1 * Hp * 4
    assert int(lib.ggpm_level_q_part_bytes(0, H)) == 0 and int(lib.ggpm_level_q_part_bytes(40, 0)) == 0


@pytest.mark.parametrize("H", HIDDEN)
def test_form_applies_to_dense_gru_levels_of_two_to_five_groups_on_fp32_mfma(H):
    """Every E1 = 2 .. 4096: the form applies exactly to dense GRU calls with 2 <= groups <= 5, one row tile and gate mode 0;
    never to LSTM or sparse calls; and ggpm_level_form_query answers the same with and without a buffer."""
    dummy = ctypes.create_string_buffer(64)
    seen = set()
    for E1 in range(2, 4097):
        form = F_.level_form(False, E1, H, training=True)
        want = int(2 <= form.groups <= MAX_GROUPS and form.rt2 == 0 and form.gate_mode == 0)
        assert _ksplit(False, E1, H) == want, (E1, form.groups)
        assert _ksplit(True, E1, H) == 0 and _ksplit(False, E1, H, sparse=True) == 0 and _ksplit(True, E1, H, sparse=True) == 0
        if want:
            assert form.fuse_fwd == 0 and form.lds_fwd_b > 0          # the level's last executed step keeps its B launch
            seen.add(form.groups)
        with_buf = F_.LevelOpts(q_part=ctypes.addressof(dummy), q_part_bytes=1 << 40)
        for lstm in (False, True):
            for sparse in (False, True):
                for training in (False, True):
                    a = F_.level_form(lstm, E1, H, sparse=sparse, training=training)
                    b = F_.level_form(lstm, E1, H, sparse=sparse, training=training, opts=with_buf)
                    assert _form_tuple(a) == _form_tuple(b)
    # (16 tiles at H = 250 in groups of at least 4: four groups at the most; H = 600 also has 6 .. 10 groups, on B launches)
    assert seen == ({2, 3, 4} if H == 250 else {2, 3, 4, 5})


def test_form_follows_the_gate_mode_and_row_tiles_of_the_call():
    """bf16 operands (gate mode 1) and two row tiles per workgroup keep their B launches; fp32 on MFMA only and forced split
    operands (mode 2 only where a level has the LDS for it: not on column groups ... unless forced) answer by their mode"""
    for H in HIDDEN:
        for E1 in (40, 817, 1361):
            for dt in range(4):
                for pn in (0, 1):
                    o = F_.LevelOpts(gate_dtype=dt, prefer_narrow=pn)
                    form = F_.level_form(False, E1, H, opts=o)
                    want = int(2 <= form.groups <= MAX_GROUPS and form.rt2 == 0 and form.gate_mode == 0)
                    assert _ksplit(False, E1, H, opts=o) == want, (H, E1, dt, pn)
            assert _ksplit(False, E1, H, opts=F_.LevelOpts(gate_dtype=1)) == 0
            assert _ksplit(False, E1, H, opts=F_.LevelOpts(prefer_narrow=1)) == 0
    assert _ksplit(False, 0, 300) == 0 and _ksplit(False, 40, 0) == 0
    assert _ksplit(False, 40, 1265) == 0          # a hidden size the level entry points refuse


def _dims(E1t, gate_dtype, rnn_type=0, H=300):
    d = EncDims()
    d.H, d.He, d.depthT, d.depthG, d.atom_size, d.n_motif, d.n_attach = H, 250, 20, 20, 38, 500, 900
    d.N1g, d.E1g, d.Kg_a, d.Kg_b = 700, 1500, 6, 6
    d.N1t, d.E1t, d.Kt_a, d.Kt_b, d.Kt_c, d.B = E1t // 2 + 1, E1t, 8, 8, 12, 32
    d.rnn_type, d.tree_chain, d.gate_dtype = rnn_type, 6, gate_dtype
    return d


def _arena(nbytes):
    return (nbytes + 255) // 256 * 256          # the arenas hand out 256-byte aligned blocks


@pytest.mark.parametrize("E1t", [571, 41, 2049])
def test_encoder_arenas_grow_by_exactly_the_tree_side_buffers(E1t):
    """ggpm_encoder_saved_bytes holds one buffer per tree-side level, ggpm_encoder_infer_bytes one for both (the forward-only
    levels share their scratch), and nothing where the form does not apply: bf16 operands, LSTM, one column group.  The
    backward arena does not move.  The layout does not depend on the gate dtype otherwise, so the bf16 size is the size
    without buffers."""
    lib = _lib.load()
    H = 300
    applies = _ksplit(False, E1t, H)
    assert applies == int(E1t < 2049)
    qb = _arena(int(lib.ggpm_level_q_part_bytes(E1t, H))) if applies else 0
    on, off = _dims(E1t, 0), _dims(E1t, 1)
    assert int(lib.ggpm_encoder_saved_bytes(ctypes.byref(on))) - int(lib.ggpm_encoder_saved_bytes(ctypes.byref(off))) == 2 * qb
    assert int(lib.ggpm_encoder_infer_bytes(ctypes.byref(on))) - int(lib.ggpm_encoder_infer_bytes(ctypes.byref(off))) == qb
    mfma = _dims(E1t, 2)
    assert int(lib.ggpm_encoder_saved_bytes(ctypes.byref(mfma))) == int(lib.ggpm_encoder_saved_bytes(ctypes.byref(on)))
    lstm_on, lstm_off = _dims(E1t, 0, rnn_type=1), _dims(E1t, 1, rnn_type=1)
    assert int(lib.ggpm_encoder_saved_bytes(ctypes.byref(lstm_on))) == int(lib.ggpm_encoder_saved_bytes(ctypes.byref(lstm_off)))
    assert int(lib.ggpm_encoder_work_bytes(ctypes.byref(on))) == int(lib.ggpm_encoder_work_bytes(ctypes.byref(off)))
