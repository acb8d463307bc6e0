"""The GRU / LSTM cell adapters (functional.GruCell / LstmCell) without a GPU: a recording stand-in for the library
checks what each wrapper of a level entry point hands to the C ABI against ``_lib.SIGNATURES``, and the parameter / gradient
order against the modules of rnn.py."""
import ctypes

import pytest
import torch

from ggpm_amd import _lib, rnn
from ggpm_amd import functional as F_

H, I, ROWS, DEPTH = 8, 12, 5, 2
HP = F_.padded_hidden(H)
STREAM = ctypes.c_void_p(0x5000)
INTS = (ctypes.c_int, ctypes.c_size_t)


class _Recorder:
    """Stands in for libggpm_hip.so: records every call and answers the size queries."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 256 if name.endswith(("_pack_floats", "_workspace_bytes")) else 0
        return fn


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda *a, **k: rec)
    return rec


def _module(kind):
    torch.manual_seed(0)
    return (rnn.LSTM if kind == "lstm" else rnn.GRU)(I, H, DEPTH)


def _cell(kind):
    m = _module(kind)
    return F_.cell_for(kind == "lstm", m.level_params(), I, H), m


def _csr():
    return F_.CSR(torch.zeros(ROWS + 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ROWS, ROWS)


def _roles(cell, save=True):
    """One argument per role of the five wrappers, on CPU tensors."""
    Hs, Cs, Qs, St = cell.alloc_state(ROWS, DEPTH, save)
    z = lambda *shape: torch.zeros(*shape)
    bufs, hid = cell.dW_buffers()
    r = dict(rows=ROWS, depth=DEPTH, X=z(cell.G, ROWS, HP), pred=_csr(), succ=_csr(), Hs=Hs, Cs=Cs, Qs=Qs, St=St,
             wpack=cell.alloc_pack(), save=save, h_in=z(ROWS, HP), c_in=z(ROWS, HP), frozen=torch.zeros(ROWS, dtype=torch.uint8),
             Xg=z(ROWS, HP), d_out=z(ROWS, HP), dc_out=z(ROWS, HP), d_in=z(ROWS, HP), dc_in=z(ROWS, HP), dX=z(cell.G, ROWS, HP),
             dW_hidden=hid, work=cell.backward_workspace(ROWS, DEPTH), weight_grads=True, opts=None, stream=STREAM)
    return r, bufs, hid


WRAPPERS = {
    "forward": ("rows depth X pred Hs Cs Qs St wpack save opts stream", "forward"),
    "sparse_forward": ("rows depth h_in c_in frozen X pred Hs Cs Qs St wpack save opts stream", "sparse_forward"),
    "backward": ("rows depth Xg pred succ Hs Cs Qs St d_out dX dW_hidden work weight_grads opts stream", "backward"),
    "weight_grads": ("rows depth Hs St work dW_hidden opts stream", "weight_grads"),
    "sparse_backward": ("rows depth frozen Xg pred succ Hs Cs Qs St d_out dc_out d_in dc_in dX dW_hidden work opts stream",
                        "sparse_backward"),
}


def _call(cell, lib, wrapper, roles, **override):
    names, entry = WRAPPERS[wrapper]
    kw = {k: roles[k] for k in names.split()}
    kw.update(override)
    del lib.calls[:]
    getattr(cell, wrapper)(**kw)
    (name, args), = [c for c in lib.calls if not c[0].endswith(("_pack_floats", "_workspace_bytes"))]
    assert name == "ggpm_%s_%s" % ("lstm" if cell.G == 4 else "gru", entry)
    return name, args


@pytest.mark.parametrize("wrapper,save", [(w, True) for w in sorted(WRAPPERS)] + [("forward", False), ("sparse_forward", False)])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_wrapper_arguments_match_the_declared_signature(lib, kind, wrapper, save):
    cell, _ = _cell(kind)
    roles, _, _ = _roles(cell, save)
    name, args = _call(cell, lib, wrapper, roles)
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes)
    for pos, (a, t) in enumerate(zip(args, argtypes)):
        if t in INTS:
            assert type(a) is int, (name, pos, a)
        else:
            assert a is None or isinstance(a, ctypes.c_void_p), (name, pos, a)
        t.from_param(a)         # what ctypes itself would accept at this position
    assert args[:3] == (ROWS, H, DEPTH) and args[-1] is STREAM


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_hidden_gradients_land_at_their_positions(lib, kind):
    """dW_hidden is (GRU) Wz_h, U_r, Wh_h, b_u / (LSTM) Wi_h, Wo_h, Wu_h, Wf_h; the GRU entry points take dbu in front of
    dWh_h, and every matrix is followed by its leading dimension."""
    cell, _ = _cell(kind)
    roles, bufs, hid = _roles(cell)
    want = [hid[0], hid[1], hid[3], hid[2]] if kind == "gru" else hid
    for wrapper in ("backward", "weight_grads", "sparse_backward"):
        _, args = _call(cell, lib, wrapper, roles)
        ptrs = [a.value for a in args if isinstance(a, ctypes.c_void_p)]
        at = [ptrs.index(t.data_ptr()) for t in want]
        assert at == sorted(at) and at[-1] - at[0] == 3, (wrapper, at)     # consecutive pointer arguments, in this order
        for t in want:
            if t.dim() == 2:
                k = [i for i, a in enumerate(args) if isinstance(a, ctypes.c_void_p) and a.value == t.data_ptr()][0]
                assert args[k + 1] == t.stride(0)
    assert [b.stride(0) for b in bufs] == [W.shape[1] for W, _ in cell.gates]
    # an explicit leading dimension (the compact atom level's per-step calls, whose hidden halves the call does not write)
    _, args = _call(cell, lib, "sparse_backward", roles, ld_dW=H)
    k = [i for i, a in enumerate(args) if isinstance(a, ctypes.c_void_p) and a.value == hid[0].data_ptr()][0]
    assert args[k + 1] == H


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_a_raw_address_and_a_tensor_give_the_same_pointer(lib, kind):
    cell, _ = _cell(kind)
    roles, _, _ = _roles(cell)
    _, by_tensor = _call(cell, lib, "sparse_forward", roles)
    csr = roles["pred"]
    raw = dict(h_in=roles["h_in"].data_ptr(), frozen=roles["frozen"].data_ptr(), Hs=roles["Hs"].data_ptr(),
               pred=(csr.rowptr.data_ptr(), csr.col), wpack=roles["wpack"].data_ptr())
    _, by_address = _call(cell, lib, "sparse_forward", roles, **raw)
    value = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a
    assert [value(a) for a in by_tensor] == [value(a) for a in by_address]
    assert F_._a(None).value is None and F_._a(roles["Hs"]).value == roles["Hs"].data_ptr()
    # without saving: no stash pointers, Cs only where the cell has one
    nosave, _, _ = _roles(cell, save=False)
    assert nosave["St"] == (None,) * 5 and (nosave["Cs"] is None) == (kind == "gru")
    assert nosave["Hs"].shape == (2, ROWS, HP) and nosave["Qs"].shape == (2, ROWS, HP)
    assert roles["Hs"].shape == (DEPTH + 1, ROWS, HP) and roles["Qs"].shape == (DEPTH, ROWS, HP)
    assert roles["St"].shape == (5, DEPTH, ROWS, HP)


def test_gru_parameter_order_is_the_modules(monkeypatch):
    cell, m = _cell("gru")
    seen = []
    monkeypatch.setattr(F_, "gru_level", lambda x, *a, **k: seen.append(a) or x)
    m.forward_padded(torch.zeros(ROWS, I), _csr())
    passed = seen[0][:7]
    assert len(cell.params) == 7 and all(p is q for p, q in zip(cell.params, passed))
    assert [id(p) for p in passed] == [id(p) for p in (m.W_z.weight, m.W_z.bias, m.W_r.weight, m.U_r.weight, m.U_r.bias,
                                                       m.W_h.weight, m.W_h.bias)]
    assert cell.G == 3 and cell.reread == 1
    assert [(id(W), b if b is None else id(b)) for W, b in cell.gates] == \
        [(id(m.W_z.weight), id(m.W_z.bias)), (id(m.W_r.weight), None), (id(m.W_h.weight), id(m.W_h.bias))]
    assert cell.U_r is m.U_r.weight and cell.b_u is m.U_r.bias
    hw = cell.hidden()
    assert [w.data_ptr() for w, _ in hw] == [m.W_z.weight.data_ptr() + 4 * I, m.U_r.weight.data_ptr(),
                                             m.W_h.weight.data_ptr() + 4 * I]
    assert [ld for _, ld in hw] == [I + H, H, I + H]
    W_arr, ld_arr = cell.hidden_weight_arrays()
    assert list(W_arr) == [w.data_ptr() for w, _ in hw] + [None] and list(ld_arr) == [I + H, H, I + H, 0]


def test_lstm_parameter_order_is_the_modules(monkeypatch):
    cell, m = _cell("lstm")
    seen = []
    monkeypatch.setattr(F_, "lstm_level", lambda x, *a, **k: seen.append(a) or (x, x))
    m.forward_padded(torch.zeros(ROWS, I), _csr())
    passed = seen[0][:8]
    assert len(cell.params) == 8 and all(p is q for p, q in zip(cell.params, passed))
    mods = (m.W_i[0], m.W_o[0], m.W[0], m.W_f[0])          # input, output, update (tanh), forget
    assert [id(p) for p in passed] == [id(p) for q in mods for p in (q.weight, q.bias)]
    assert cell.G == 4 and cell.reread == 3 and cell.U_r is None and cell.b_u is None
    assert [(id(W), id(b)) for W, b in cell.gates] == [(id(q.weight), id(q.bias)) for q in mods]
    hw = cell.hidden()
    assert [w.data_ptr() for w, _ in hw] == [q.weight.data_ptr() + 4 * I for q in mods] and [ld for _, ld in hw] == [I + H] * 4
    W_arr, ld_arr = cell.hidden_weight_arrays()
    assert list(W_arr) == [w.data_ptr() for w, _ in hw] and list(ld_arr) == [I + H] * 4


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_gradient_tuple_follows_the_parameter_order(kind):
    cell, _ = _cell(kind)
    bufs, hid = cell.dW_buffers()
    dbs = [None if b is None else torch.zeros(H) for _, b in cell.gates]
    grads = cell.grads(bufs, hid, dbs)
    assert len(grads) == len(cell.params)
    assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in cell.params]
    if kind == "gru":       # W_z, b_z, W_r (no bias slot), U_r, b_u, W_h, b_h
        want = (bufs[0], dbs[0], bufs[1], hid[1], hid[3], bufs[2], dbs[2])
        assert dbs[1] is None
        assert hid[0].data_ptr() == bufs[0].data_ptr() + 4 * I and hid[2].data_ptr() == bufs[2].data_ptr() + 4 * I
    else:
        want = (bufs[0], dbs[0], bufs[1], dbs[1], bufs[2], dbs[2], bufs[3], dbs[3])
        assert [h.data_ptr() for h in hid] == [b.data_ptr() + 4 * I for b in bufs]
    assert all(g is w for g, w in zip(grads, want))
