"""GPU: the GRU / LSTM level kernels with saturated gates, and with one NaN in a parameter of the gather sigmoid.

Saturation (tests/level_extreme_cases.py: a third and more of the gather-sigmoid arguments beyond 17, one in a hundred
and more beyond the clamp at 88; tests/test_level_extremes_cpu.py holds the inputs to that): forward + backward on
fp32 MFMA and on split operands, and a sparse forward, against the fp64 oracle at the project's 1e-4 bar.

Poison: a NaN in W_r, U_r, b_u (GRU) or W_f, b_f (LSTM) has one way into h, the sigmoid of the gather phase.  It must
arrive: every element the recurrence over the REAL predecessor lists carries it to is NaN, every other element is
bit-identical to the same call without the NaN.  (The padded oracle is no guide here: its h * mask and its pad slots
compute NaN * 0; the kernels rightly skip empty lists and the h = 0 depth.)"""
import numpy as np
import pytest
import torch

import level_extreme_cases as X
from golden_utils import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4   # BASELINE.json: outputs / losses within 1e-4 fp32 relative


def _dev():
    return torch.device("cuda:0")


def _module(cell, H, depth, sd, gate_dtype=None):
    from ggpm_amd import rnn as R
    mod = (R.GRU if cell == "GRU" else R.LSTM)(X.I, H, depth).to(_dev())
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    if gate_dtype is not None:
        mod.gate_dtype = gate_dtype
    return mod


# ------------------------------------------------------------------------------------------------------- saturation
_ORACLE = {}


def _oracle(cell, shape):
    """the fp64 and the fp32 run of the oracle on the saturating inputs: computed once per (cell, shape), never written to"""
    if (cell, shape) not in _ORACLE:
        E, _, H, depth = shape
        sd, x, bgraph, w = X.saturating(cell, E, H)
        runs = tuple(X.oracle_dense(cell, sd, x, bgraph, w, depth, dt) for dt in (torch.float64, torch.float32))
        for r in runs:
            for a in r.values():
                a.setflags(write=False)
        _ORACLE[cell, shape] = runs
    return _ORACLE[cell, shape]


def _compare(what, got, want64, want32):
    assert sorted(got) == sorted(want64)
    for k in sorted(got):
        e, o = rel_err(got[k], want64[k]), rel_err(want32[k], want64[k])
        print("%s %-14s HIP-fp64 %.2e   oracle32-fp64 %.2e" % (what, k, e, o))
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert (got["h"][0] == 0).all()
    for k in got:
        assert rel_err(got[k], want64[k]) < TOL, (k, rel_err(got[k], want64[k]))


@pytest.mark.parametrize("gate_dtype", ["f32_mfma", "f32_split"])
@pytest.mark.parametrize("shape", X.SHAPES, ids=X.shape_id)
@pytest.mark.parametrize("cell", X.CELLS)
def test_saturated_level_matches_fp64(cell, shape, gate_dtype):
    """rnn.GRU / rnn.LSTM forward + backward with saturated gates: finite, row 0 zero, h, c, dx and every parameter
    gradient within 1e-4 of the fp64 oracle"""
    E, _, H, depth = shape
    sd, x, bgraph, w = X.saturating(cell, E, H)
    mod = _module(cell, H, depth, sd, gate_dtype)
    xg = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    out = mod(xg, torch.from_numpy(bgraph).to(_dev()))
    h = out if cell == "GRU" else out[0]
    (h * torch.from_numpy(w).to(_dev())).sum().backward()
    got = dict({k: v.grad.cpu().numpy() for k, v in mod.named_parameters()}, h=h.detach().cpu().numpy(),
               dx=xg.grad.cpu().numpy())
    if cell == "LSTM":
        got["c"] = out[1].detach().cpu().numpy()
        assert (got["c"][0] == 0).all()
    want64, want32 = _oracle(cell, shape)
    _compare("saturated %s %s %s" % (cell, X.shape_id(shape), gate_dtype), got, want64, want32)


@pytest.mark.parametrize("cell", X.CELLS)
def test_saturated_sparse_forward_matches_fp64(cell):
    """sparse_forward on the H = 300 shape with the same scaling: the recomputed rows and the rows passed through"""
    from oracle import ref_encoder as ref
    E, _, H, depth = X.SHAPES[1]
    sd, (h, c, submess, x, bg, _) = X.saturating_sparse(cell, E, H)
    mod = _module(cell, H, depth, sd)
    ht, ct = (torch.from_numpy(a).to(_dev()).requires_grad_(True) for a in (h, c))
    xt, sm, bgt = (torch.from_numpy(a).to(_dev()) for a in (x, submess, bg))
    if cell == "GRU":
        got = {"h": mod.sparse_forward(ht, xt, sm, bgt).detach().cpu().numpy()}
    else:
        ho, co = mod.sparse_forward((ht, ct), xt, sm, bgt)
        got = {"h": ho.detach().cpu().numpy(), "c": co.detach().cpu().numpy()}
    want = []
    for dt in (torch.float64, torch.float32):
        p = {"rnn." + k: torch.from_numpy(v).to(dt) for k, v in sd.items()}
        h_, c_, x_ = (torch.from_numpy(a).to(dt) for a in (h, c, x))
        sm_, bg_ = torch.from_numpy(submess), torch.from_numpy(bg)
        if cell == "GRU":
            want.append({"h": ref.gru_sparse_forward(p, "rnn.", h_, x_, sm_, bg_, depth).numpy()})
        else:
            ro, rc = ref.lstm_sparse_forward(p, "rnn.", h_, c_, x_, sm_, bg_, depth)
            want.append({"h": ro.numpy(), "c": rc.numpy()})
    _compare("saturated sparse %s %s" % (cell, X.shape_id(X.SHAPES[1])), got, *want)


# ----------------------------------------------------------------------------------------------------------- poison
def _forward(cell, H, depth, sd, x, bgraph, stash):
    """One forward -> (h, c or None) as arrays.  ``stash``: parameters and input require gradients, so the level keeps its
    stashes (the STASH kernel instantiations); else a frozen module under no_grad (the two-slot forward-only ones)."""
    mod = _module(cell, H, depth, sd)
    xg = torch.from_numpy(x).to(_dev())
    bg = torch.from_numpy(bgraph).to(_dev())
    if stash:
        out = mod(xg.requires_grad_(True), bg)
        assert (out if cell == "GRU" else out[0]).requires_grad
    else:
        mod.requires_grad_(False)
        with torch.no_grad():
            out = mod(xg, bg)
    torch.cuda.synchronize()
    if cell == "GRU":
        return out.detach().cpu().numpy(), None
    return out[0].detach().cpu().numpy(), out[1].detach().cpu().numpy()


_CLEAN = {}


def _clean_run(cell, E, H, depth, stash):
    if (cell, E, H, depth, stash) not in _CLEAN:
        sd, x, bgraph, _ = X.clean(cell, E, H)
        res = _forward(cell, H, depth, sd, x, bgraph, stash)
        assert all(np.isfinite(a).all() for a in res if a is not None)
        _CLEAN[cell, E, H, depth, stash] = res
    return _CLEAN[cell, E, H, depth, stash]


@pytest.mark.parametrize("stash", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("depth", X.POISON_DEPTHS, ids=lambda d: "depth%d" % d)
@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "E%d-H%d" % (s[0], s[2]))
@pytest.mark.parametrize("poison", X.POISON, ids=X.poison_id)
def test_nan_in_a_gather_sigmoid_parameter_reaches_h(poison, shape, depth, stash):
    """GRU: every row with a real predecessor is NaN in all H columns.  LSTM: such a row is NaN in column j of h and c
    at depth 2; from depth 3 on in every column where one of its predecessors had predecessors (s = sum h then carries the
    NaN into i, o, u), in column j otherwise.  Rows without predecessors, and row 0, are bit-identical to the clean run."""
    cell, name, half = poison
    E, _, H, _ = shape
    sd, x, bgraph, _ = X.clean(cell, E, H)
    j, index = X.poison_element(cell, name, half, H)
    want_h, want_c = _clean_run(cell, E, H, depth, stash)
    got_h, got_c = _forward(cell, H, depth, X.poisoned(sd, name, index), x, bgraph, stash)
    nan_h, nan_c = X.poison_nan_masks(cell, bgraph, H, depth, j)
    has = (bgraph > 0).any(axis=1)
    # the issue's statement of the pattern, on top of the element-wise mask: rows with predecessors carry the NaN ...
    assert has.any() and nan_h[has][:, j].all() and not nan_h[~has].any()
    if cell == "GRU":
        assert nan_h[has].all()
    for what, got, want, nan in (("h", got_h, want_h, nan_h), ("c", got_c, want_c, nan_c)):
        if got is None:
            continue
        missing = nan & ~np.isnan(got)
        assert not missing.any(), "%s: %d of %d elements that must be NaN are finite, e.g. row %d col %d = %r" % (
            what, missing.sum(), nan.sum(), *np.argwhere(missing)[0], got[tuple(np.argwhere(missing)[0])])
        # ... and nothing else changed by a bit
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), what
        assert (got[0] == 0).all(), what
