"""Inputs that drive the GRU / LSTM level kernels' gate math where the other level tests never go: saturated gates, and
one NaN in one parameter of the gather sigmoid.

Every other level test draws x from a unit normal and Xavier weights: no gate pre-activation beyond about 4, no sigmoid
argument beyond 17.  ``saturating`` scales the same draws so that a third of the gather-sigmoid arguments (x_r + q of the
GRU, x_f + q_f of the LSTM) lie beyond 17 -- where the result is 1 or 0 to fp32 and ``1 - r`` cancels -- and more than one
in a hundred beyond the clamp at 88 of ``ggpm_fsigmoid_acc`` (csrc/common.h); tests/test_level_extremes_cpu.py holds the
inputs to that, tests/test_gpu_level_extremes.py runs them.  ``POISON`` lists the parameters whose only way into h is the
gather sigmoid, and ``poison_nan_masks`` derives from the recurrence over the REAL predecessor lists which elements of the
result a NaN in one of them must reach.
"""
import numpy as np

import level_form_cases as C

I = C.I
SHAPES = [(40, I, 24, 3), (333, I, 300, 3)]          # (E, I, H, depth): one block of one tile; 21 row tiles x 19 column tiles
CELLS = ("GRU", "LSTM")
WEIGHT_SCALE, X_SCALE, ROW_SCALE = 8.0, 8.0, 4.0


def shape_id(s):
    return "E%d-H%d-d%d" % (s[0], s[2], s[3])


def _seed(cell, E, H):
    # (the LSTM at H = 300 is the thinnest: 0.8 .. 1.5 % of its arguments beyond 88 over a dozen seeds, 1.5 % with this
    # one; the oracle's fp32 run lands 5e-6 .. 1.6e-5 from fp64 over the same seeds, 8.7e-6 with this one)
    return 8 * E + H + (1 if cell == "LSTM" else 0)


def _weights(cell, E, H):
    from ggpm_amd.params import rnn_param_shapes, seeded_state_dict
    return seeded_state_dict(rnn_param_shapes(cell, I, H), seed=_seed(cell, E, H))


def _scale_x(x):
    x = x * np.float32(X_SCALE)
    x[5::16] *= np.float32(ROW_SCALE)
    return x


def clean(cell, E, H):
    """-> state dict, x [E + 1, I], bgraph [E + 1, K + 1], the cotangent on h: inputs and weights at scale 1"""
    rs = np.random.RandomState(_seed(cell, E, H))
    x, bgraph = C.random_level(rs, E, I)
    return _weights(cell, E, H), x, bgraph, rs.standard_normal((E + 1, H)).astype(np.float32)


def saturating(cell, E, H):
    """``clean`` with every weight and bias times 8, x times 8, rows x[5::16] times a further 4"""
    sd, x, bgraph, w = clean(cell, E, H)
    return {k: v * np.float32(WEIGHT_SCALE) for k, v in sd.items()}, _scale_x(x), bgraph, w


def saturating_sparse(cell, E, H):
    """-> state dict, golden_utils.sparse_inputs (h, c, submess, x, bgraph, cotangents) of a call that recomputes a quarter
    of the rows, with the same scaling of the weights and of x (the incoming state stays: |h| < 1 in a real model)"""
    from golden_utils import sparse_inputs
    h, c, submess, x, bg, coef = sparse_inputs(E + 1, I, H, (E + 1) // 4, C.K, _seed(cell, E, H))
    sd = {k: v * np.float32(WEIGHT_SCALE) for k, v in _weights(cell, E, H).items()}
    return sd, (h, c, submess, _scale_x(x), bg, coef)


def gather_sigmoid_arguments(cell, sd, x, bgraph, depth):
    """Every argument the gather sigmoid sees in fp64: x_r[e] + q[p] (GRU), x_f[e] + q_f[p] (LSTM) for every message e, every
    real predecessor p of e and every depth after the first (h = 0 at the first: the kernels walk no list there)."""
    import torch
    from oracle import ref_encoder as ref
    p = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    trace = []
    ref.rnn_forward(p, "", cell, torch.from_numpy(x).double(), torch.from_numpy(bgraph), depth, trace=trace)
    x64 = x.astype(np.float64)
    if cell == "GRU":
        xa = x64 @ sd["W_r.weight"].astype(np.float64).T
        Wq, bq = sd["U_r.weight"].astype(np.float64), sd["U_r.bias"].astype(np.float64)
    else:
        Wf = sd["W_f.0.weight"].astype(np.float64)
        xa = x64 @ Wf[:, :I].T + sd["W_f.0.bias"].astype(np.float64)
        Wq, bq = Wf[:, I:], 0.0
    e, slot = np.nonzero(bgraph > 0)
    pred = bgraph[e, slot]
    return np.concatenate([(xa[e] + (h.numpy() @ Wq.T + bq)[pred]).ravel() for h in trace[:depth - 1]])


def oracle_dense(cell, sd, x, bgraph, w, depth, dtype):
    """forward + backward of the oracle -> {tensor name: array} (h, c for the LSTM, dx, every parameter gradient)"""
    import torch
    from oracle import ref_encoder as ref
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = torch.from_numpy(x).to(dtype).requires_grad_(True)
    bg = torch.from_numpy(bgraph)
    if cell == "GRU":
        h, res = ref.gru_forward(p, "", xr, bg, depth), {}
    else:
        h, c = ref.lstm_forward(p, "", xr, bg, depth)
        res = {"c": c.detach().numpy()}
    (h * torch.from_numpy(w).to(dtype)).sum().backward()
    res.update({k: v.grad.numpy() for k, v in p.items()}, h=h.detach().numpy(), dx=xr.grad.numpy())
    return res


# ------------------------------------------------------------------------------------------------------------ poison
# (cell, parameter, which half of its columns, bias?): a NaN here enters h only through the gather sigmoid
POISON = [("GRU", "W_r.weight", "x"), ("GRU", "U_r.weight", "h"), ("GRU", "U_r.bias", None),
          ("LSTM", "W_f.0.weight", "x"), ("LSTM", "W_f.0.weight", "h"), ("LSTM", "W_f.0.bias", None)]
POISON_DEPTHS = (2, 3)


def poison_id(p):
    return "%s-%s%s" % (p[0], p[1], "" if p[2] is None else "-" + p[2] + "half")


def poison_element(cell, name, half, H):
    """-> (j, index into the parameter): gate column j (in the last, partly padded 16-column tile at H = 300), and an input
    column inside the x-half or the h-half"""
    j = H - 3
    if half is None:
        return j, (j,)
    k = 3 if half == "x" else 7
    return j, (j, k + (I if (cell == "LSTM" and half == "h") else 0))


def poisoned(sd, name, index):
    out = {k: v.copy() for k, v in sd.items()}
    out[name][index] = np.nan
    return out


def poison_nan_masks(cell, bgraph, H, depth, j):
    """Which elements of (h, c) a NaN in column j of the gather sigmoid's argument reaches after ``depth`` steps, from the
    recurrence over the real predecessor lists (bool [E1, H] each; c all False for the GRU).

    The first step walks no list (h = 0).  From the second on a message with at least one real predecessor evaluates the
    sigmoid, NaN in column j.  GRU: g = sum r h is NaN in column j and tanh(W_h [x, g]) in every column.  LSTM: c' = i u + sum f c
    is NaN in column j, h' = o tanh(c') too; a NaN anywhere in s = sum h (a predecessor that itself had predecessors one step
    earlier) makes i, o, u and so the whole row NaN.  A message without predecessors never sees the NaN, row 0 is zero."""
    real = bgraph > 0
    has = real.any(axis=1)
    nh = np.zeros((bgraph.shape[0], H), dtype=bool)
    nc = np.zeros_like(nh)
    for d in range(2, depth + 1):
        if cell == "GRU":
            nh = np.repeat(has[:, None], H, axis=1)
            continue
        s_nan = (nh[bgraph] & real[:, :, None]).any(axis=1)
        c_nan = (nc[bgraph] & real[:, :, None]).any(axis=1)
        new = c_nan | s_nan.any(axis=1)[:, None]
        new[has, j] = True
        nh, nc = new, new.copy()
    nh[0] = False
    nc[0] = False
    return nh, nc
