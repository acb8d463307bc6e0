"""What the GPU tests of the level forms share (tests/test_gpu_level_forms.py, tests/test_gpu_level_option_forms.py,
tests/test_gpu_parity.py): the module and the oracle runs of a case of tests/level_form_cases.py, the two fp32 bars against
the fp64 oracle, the row-wise criteria of the bf16 kernels against the bf16 oracle, and a level call driven through the cell
adapters of ggpm_amd/functional.py under explicit ``ggpm_level_opts`` from NaN-filled, guarded buffers."""
import ctypes
import time

import numpy as np
import torch

import level_form_cases as C
from golden_utils import rel_err

TOL = 1e-4   # BASELINE.json: outputs / losses within 1e-4 fp32 relative
BF16_STEP_TOL = 1e-3 # ... parameter gradients of one level over 2-3 depth steps (flipped roundings included, not yet amplified)
# the rows of a bf16 level against the bf16 oracle (test_bf16_level_kernels_match_the_bf16_oracle states why): rows without a
# flipped rounding within BF16_ROW_TOL of the tensor's scale, at least BF16_ROW_FRAC of the rows; the median and the worst row
BF16_ROW_TOL = 2e-5
BF16_ROW_FRAC = {"h": 0.9, "dx": 0.7}
BF16_ROW_FRAC_STORED = {"h": 0.75, "dx": 0.5}
BF16_ROW_MEDIAN, BF16_ROW_MEDIAN_STORED = 2e-6, 5e-6      # (measured: <= 2.6e-6 at H = 600, 0.0 for the state at every size)
BF16_ROW_WORST, BF16_ROW_WORST_STORED = 2e-3, 6e-3
BF16_RAN = 1e-5      # the bf16 state is at least this far from the fp32 state: the bf16 path really ran


def dev():
    return torch.device("cuda:0")


def module(case, sd):
    from ggpm_amd import rnn as R
    mod = (R.GRU if case.cell == "GRU" else R.LSTM)(C.I, case.H, case.depth).to(dev())
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return mod


def check(case, form, got, want64, want32, t0):
    """Both bars on every tensor; prints the case's worst distances (HIP vs fp64, the oracle's fp32 run vs fp64, and the
    largest share of the second bar any tensor used)."""
    assert sorted(got) == sorted(want64) == sorted(want32)
    hip = {k: rel_err(got[k], want64[k]) for k in got}
    o32 = {k: rel_err(want32[k], want64[k]) for k in got}
    share = {k: hip[k] / (3.0 * o32[k] + 1e-6) for k in got}
    kh, ko, ks = (max(d, key=d.get) for d in (hip, o32, share))
    print("level form %-26s form %-22s HIP-fp64 %.2e (%s)  oracle32-fp64 %.2e (%s)  share of 3x+1e-6 %.2f (%s)  %.2f s"
          % (C.case_id(case), C.reduced(form), hip[kh], kh, o32[ko], ko, share[ks], ks, time.perf_counter() - t0))
    for k in got:
        assert hip[k] < TOL, (k, hip[k])
        assert hip[k] <= 3.0 * o32[k] + 1e-6, (k, hip[k], o32[k])


def dense_oracle(case, sd, x, bgraph, w, dtype, gate_dtype="f32"):
    from oracle import ref_encoder as ref
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = torch.from_numpy(x).to(dtype).requires_grad_(True)
    href = ref.rnn_forward(p, "", case.cell, xr, torch.from_numpy(bgraph), case.depth, gate_dtype=gate_dtype)
    (href * torch.from_numpy(w).to(dtype)).sum().backward()
    return dict({k: v.grad.numpy() for k, v in p.items()}, h=href.detach().numpy(), dx=xr.grad.numpy())


def sparse_oracle(case, sd, inputs, dtype, gate_dtype="f32"):
    from oracle import ref_encoder as ref
    h, c, submess, x, bg, coef = inputs
    p = {"rnn." + k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    hr, cr, xr = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (h, c, x))
    cf = torch.from_numpy(coef).to(dtype)
    sm, bgt = torch.from_numpy(submess), torch.from_numpy(bg)
    if case.cell == "GRU":
        ro = ref.gru_sparse_forward(p, "rnn.", hr, xr, sm, bgt, case.depth, gate_dtype=gate_dtype)
        (cf[0] * ro).sum().backward()
        res = {}
    else:
        ro, rc = ref.lstm_sparse_forward(p, "rnn.", hr, cr, xr, sm, bgt, case.depth, gate_dtype=gate_dtype)
        ((cf[0] * ro).sum() + (cf[1] * rc).sum()).backward()
        res = {"c": rc.detach().numpy(), "dc_in": cr.grad.numpy()[1:]}
    # (row 0 of the incoming-state gradients: the pad row, see test_sparse_forward_matches_reference_golden)
    res.update({k[4:]: v.grad.numpy() for k, v in p.items()}, h=ro.detach().numpy(), dh_in=hr.grad.numpy()[1:],
               dx=xr.grad.numpy())
    return res


def bf16_oracle_mode(lib, H, contraction_rows, stored):
    """The oracle's gate_dtype for a level on bf16 operands: "bf16s" under bf16 storage; "bf16w" where the level's shortest
    weight-gradient contraction (``contraction_rows`` rows) takes the bf16 tall kernel, "bf16" where it falls back to
    fp32 operands (include/ggpm_hip.h: ggpm_gemm_tn_bf16)."""
    if stored:
        return "bf16s"
    return "bf16w" if lib.ggpm_gemm_tn_bf16_applies(H, H, contraction_rows) else "bf16"


def check_bf16_level(label, got16, got32, want, mode, params, rows=(("h", "h", None), ("dx", "dx", None))):
    """The bf16 kernels of ONE level against the oracle that rounds the same operands at the same points (``want``, run in
    ``mode``), with the fp32 HIP result of the same call beside them (``got32``).  ``rows``: (tensor, kind, row subset or
    None) of the tensors held row-wise -- kind "h" for a state, "dx" for a gradient the backward gather spreads -- the
    unflipped rows agree to fp32 noise; ``params``: the tensors held norm-wise within BF16_STEP_TOL and at most a third of
    the bf16 -> fp32 distance.  Prints every figure before it asserts."""
    stored = mode == "bf16s"
    shift = {k: rel_err(got16[k], got32[k]) for k in want}
    report, figures = [], []
    for k, kind, sel in rows:                    # row-wise: unflipped rows agree to fp32 noise
        g, w = (got16[k], want[k]) if sel is None else (got16[k][sel], want[k][sel])
        scale = np.abs(want[k]).max()
        row = np.abs(g - w).max(axis=1) / scale
        med, frac, worst = float(np.median(row)), float((row <= BF16_ROW_TOL).mean()), float(row.max())
        report.append("%s rows: median %.1e, %.1f%% within 2e-5, worst %.1e" % (k, med, 100 * frac, worst))
        figures.append((k, kind, med, frac, worst))
    errs = {k: rel_err(got16[k], want[k]) for k in params}
    worst_k = max(errs, key=errs.get)
    print("bf16 level %s (weight-gradient operands %s): %s; parameter gradients worst %.2e (%s) at a bf16 -> fp32 distance "
          "of %.2e; state bf16 -> fp32 %.2e" % (label, mode, "; ".join(report), errs[worst_k], worst_k, shift[worst_k], shift["h"]))
    assert shift["h"] > BF16_RAN                 # the bf16 path really ran
    for k, kind, med, frac, worst in figures:
        # (a flipped row reaches its predecessors through the backward gather: more dx rows than h rows are touched)
        # (bf16 storage: what a flip moves is a STORED value, by one bf16 ulp of itself, i.e. up to 2^-8 of the tensor's scale)
        # and every stored array is one more rounding point per element and depth step: more rows meet a flip)
        worst_tol = BF16_ROW_WORST_STORED if stored else BF16_ROW_WORST
        frac_min = BF16_ROW_FRAC_STORED if stored else BF16_ROW_FRAC
        med_tol = BF16_ROW_MEDIAN_STORED if stored else BF16_ROW_MEDIAN
        assert med <= med_tol and frac >= frac_min[kind] and worst <= worst_tol, (k, med, frac, worst)
        # What the relaxed row fractions above still pin: a wrong rounding point, rounding mode, operand
        # order or accumulation moves EVERY row.  Under bf16 storage a state row without a flipped rounding is BIT-EQUAL to
        # the oracle (both round the same fp32 value to the same bf16), so the median row distance is exactly zero -- asserted.
        if stored and k == "h":
            assert med == 0.0, ("bf16 storage: the median state row must be bit-equal to the oracle", med)
    for k, e in errs.items():
        assert e <= BF16_STEP_TOL and e <= max(shift[k] / 3.0, 2e-5), (k, e, shift[k])


# ---- a level call through the cell adapters (functional.cell_for), under explicit ggpm_level_opts
class Buffers:
    """Device buffers a level call writes, as the autograd nodes allocate them with torch.empty -- here NaN-filled, with
    GUARD NaN floats before and after each that must still be NaN afterwards: a call reads nothing it did not write, and
    writes nothing outside the sizes the library states."""
    GUARD = 256

    def __init__(self):
        self.held = []

    def new(self, *shape):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * self.GUARD,), float("nan"), dtype=torch.float32, device=dev())
        self.held.append(flat)
        return flat[self.GUARD:self.GUARD + n].view(*shape)

    def like_empty(self, t):
        """a tensor the adapters allocated with torch.empty, poisoned in place"""
        return t.fill_(float("nan"))

    def assert_guards(self):
        torch.cuda.synchronize()
        for flat in self.held:
            g = self.GUARD
            assert bool(torch.isnan(flat[:g]).all()) and bool(torch.isnan(flat[-g:]).all()), "a level call wrote outside its buffer"


def _names_in_level_order(mod):
    names = {id(p): n for n, p in mod.named_parameters()}
    return [names[id(p)] for p in mod.level_params()]


def _cell(case, mod):
    from ggpm_amd import functional as F_
    return F_.cell_for(case.cell == "LSTM", [p.detach() for p in mod.level_params()], C.I, case.H)


def _state(bufs, cell, rows, depth, save):
    """functional._Cell.alloc_state, poisoned"""
    n, Hp = (depth + 1 if save else 2), cell.Hp
    Hs = bufs.new(n, rows, Hp)
    Cs = bufs.new(n, rows, Hp) if cell.G == 4 else None
    Qs = bufs.new(depth if save else 2, rows, Hp)
    return Hs, Cs, Qs, (bufs.new(5, depth, rows, Hp) if save else (None,) * 5)


def _workspace(bufs, cell, rows, depth):
    lib = cell.lib
    wb = int((lib.ggpm_lstm_backward_workspace_bytes if cell.G == 4 else lib.ggpm_gru_backward_workspace_bytes)(rows, cell.H, depth))
    return bufs.new((wb + 3) // 4)


def _ref(opts):
    return None if opts is None else ctypes.byref(opts)


def _param_grads(bufs, cell, mod, dX, x, rows, hid, gate_bufs):
    from ggpm_amd import functional as F_
    grads = cell.grads(gate_bufs, hid, cell.input_half_grads(dX, x, F_._ld(x), rows, gate_bufs))
    return {n: g.cpu().numpy() for n, g in zip(_names_in_level_order(mod), grads)}


def dense_by_adapters(case, mod, x, bgraph, w, opts, train=True, h_out=False):
    """functional._level_forward / _level_backward restated with ``opts`` (a functional.LevelOpts or None) on poisoned
    buffers.  train: forward with stashes + backward -> ({h, dx, every parameter gradient} as numpy, the device tensors
    (h, c or None) [E1, Hp] of the last slot); else the
    forward without stashes -> (h, c or None) as device tensors [E1, Hp] out of the two ping-pong slots, or, with
    ``h_out``, out of ggpm_level_opts.h_out / c_out (the forward-only form that keeps bf16 storage)."""
    from ggpm_amd import functional as F_
    bufs, cell = Buffers(), _cell(case, mod)
    E1, depth, H, Hp = case.E1, case.depth, case.H, cell.Hp
    xg = torch.from_numpy(x).to(dev())
    pred = F_.csr_from_padded(torch.from_numpy(bgraph).to(dev()), ncols=E1)
    X = bufs.new(cell.G, E1, Hp)
    cell.project_inputs(xg, F_._ld(xg), E1, X)
    wpack = bufs.new(cell.pack_floats())
    Hs, Cs, Qs, St = _state(bufs, cell, E1, depth, train)
    if h_out:
        assert not train
        opts = F_.LevelOpts() if opts is None else opts
        ho, co = bufs.new(E1, Hp), (bufs.new(E1, Hp) if Cs is not None else None)
        opts.h_out, opts.c_out = ho.data_ptr(), (co.data_ptr() if co is not None else None)
    cell.forward(rows=E1, depth=depth, X=X, pred=pred, Hs=Hs, Cs=Cs, Qs=Qs, St=St, wpack=wpack, save=train, opts=_ref(opts))
    if not train:
        bufs.assert_guards()
        if h_out:
            opts.h_out = opts.c_out = None
            return ho, co
        assert Hs.shape[0] == 2      # the two-slot ping-pong
        return Hs[depth & 1], (Cs[depth & 1] if Cs is not None else None)
    dHD = torch.zeros(E1, Hp, device=dev())
    dHD[:, :H] = torch.from_numpy(w).to(dev())
    dX = bufs.new(cell.G, E1, Hp)
    gate_bufs, hid = cell.dW_buffers()
    for t in list(gate_bufs) + [t for t in hid if t._base is None]:
        bufs.like_empty(t)
    work = _workspace(bufs, cell, E1, depth)
    cell.backward(rows=E1, depth=depth, Xg=X[cell.reread], pred=pred, succ=pred.T, Hs=Hs, Cs=Cs, Qs=Qs, St=St, d_out=dHD,
                  dX=dX, dW_hidden=hid, work=work, weight_grads=True, opts=_ref(opts))
    got = _param_grads(bufs, cell, mod, dX, xg, E1, hid, gate_bufs)
    got.update(h=Hs[depth][:, :H].cpu().numpy(), dx=cell.input_grad(dX, xg, E1).cpu().numpy())
    bufs.assert_guards()
    assert all(np.isfinite(v).all() for v in got.values()), "a poisoned element reached a result"
    return got, (Hs[depth], Cs[depth] if Cs is not None else None)


def sparse_by_adapters(case, mod, inputs, opts, train=True):
    """functional._sparse_forward / _sparse_backward restated with ``opts`` on poisoned buffers.  train -> ({h, c, dh_in,
    dc_in, dx, every parameter gradient} as tests/test_gpu_level_forms.py names them, the device tensors (h, c or None) of
    the last slot); else -> (h, c or None), device
    tensors [E1, Hp] out of the two ping-pong slots."""
    from ggpm_amd import functional as F_
    bufs, cell = Buffers(), _cell(case, mod)
    E1, depth, H, Hp, ms = case.E1, case.depth, case.H, cell.Hp, case.ms
    h, c, submess, x, bg, coef = inputs
    lstm = cell.G == 4
    xs, sm, bgt, cf = (torch.from_numpy(a).to(dev()) for a in (x, submess, bg, coef))
    hp = F_._as_padded_state(torch.from_numpy(h).to(dev()), H, Hp)
    cp = F_._as_padded_state(torch.from_numpy(c).to(dev()), H, Hp) if lstm else None
    frozen, pred, _ = F_._sparse_structure(E1, sm, bgt)
    Xs = bufs.new(cell.G, ms, Hp)
    cell.project_inputs(xs, F_._ld(xs), ms, Xs)
    X = torch.zeros(cell.G, E1, Hp, device=dev())
    X.index_copy_(1, sm, Xs)
    wpack = bufs.new(cell.pack_floats())
    Hs, Cs, Qs, St = _state(bufs, cell, E1, depth, train)
    cell.sparse_forward(rows=E1, depth=depth, h_in=hp, c_in=cp, frozen=frozen, X=X, pred=pred, Hs=Hs, Cs=Cs, Qs=Qs, St=St,
                        wpack=wpack, save=train, opts=_ref(opts))
    if not train:
        bufs.assert_guards()
        return Hs[depth & 1], (Cs[depth & 1] if lstm else None)
    dHD, dCD = torch.zeros(E1, Hp, device=dev()), (torch.zeros(E1, Hp, device=dev()) if lstm else None)
    dHD[:, :H] = cf[0]
    if lstm:
        dCD[:, :H] = cf[1]
    dHin, dCin = bufs.new(E1, Hp), (bufs.new(E1, Hp) if lstm else None)
    dX = bufs.new(cell.G, E1, Hp)
    gate_bufs, hid = cell.dW_buffers()
    for t in list(gate_bufs) + [t for t in hid if t._base is None]:
        bufs.like_empty(t)
    work = _workspace(bufs, cell, E1, depth)
    cell.sparse_backward(rows=E1, depth=depth, frozen=frozen, Xg=X[cell.reread], pred=pred, succ=pred.T, Hs=Hs, Cs=Cs, Qs=Qs,
                         St=St, d_out=dHD, dc_out=dCD, d_in=dHin, dc_in=dCin, dX=dX, dW_hidden=hid, work=work, opts=_ref(opts))
    dXs = dX.index_select(1, sm)
    got = _param_grads(bufs, cell, mod, dXs, xs, ms, hid, gate_bufs)
    got.update(h=Hs[depth][:, :H].cpu().numpy(), dh_in=dHin[1:, :H].cpu().numpy(), dx=cell.input_grad(dXs, xs, ms).cpu().numpy())
    if lstm:
        got.update(c=Cs[depth][:, :H].cpu().numpy(), dc_in=dCin[1:, :H].cpu().numpy())
    bufs.assert_guards()
    assert all(np.isfinite(v).all() for v in got.values()), "a poisoned element reached a result"
    return got, (Hs[depth], Cs[depth] if Cs is not None else None)
