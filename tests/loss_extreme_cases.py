"""Inputs and fp64 references of the loss kernels (csrc/losses.hip) at large logits: softmax cross entropy with logits of
standard deviation 30 under mask rows of -1000, BCE at logits of +-100.  Shared by tests/test_loss_extremes_cpu.py (torch
fp32 on the CPU stays well inside the bars) and test_softmax_ce_and_bce_kernels_at_large_logits (tests/test_gpu_parity.py)."""
import numpy as np

SHAPES = [(5, 64), (257, 33), (4, 2100)]          # (M, N): one block; two trips of the row-sum loop; 33 trips of the class loop
LOGIT_SCALE, MASK_VALUE, MASK_ROWS, UPSTREAM = 30.0, -1000.0, 6, 1.7
LOSS_RTOL, GRAD_ATOL = 2e-5, 2e-6                # the bars of test_softmax_ce_and_bce_kernels_against_torch


def ce_inputs(M, N):
    """-> logits [M, N] fp32, labels [M], mask [MASK_ROWS, N] (0 / -1000), mask_row [M]; a row's label is never masked"""
    rs = np.random.RandomState(M * 1000 + N)
    x = (LOGIT_SCALE * rs.standard_normal((M, N))).astype(np.float32)
    labels = rs.randint(0, N, size=M).astype(np.int64)
    mask = ((rs.random_sample((MASK_ROWS, N)) > 0.5) * MASK_VALUE).astype(np.float32)
    mask_row = rs.randint(0, MASK_ROWS, size=M).astype(np.int64)
    mask[mask_row, labels] = 0.0
    return x, labels, mask, mask_row


def ce_reference(x, labels, mask, mask_row):
    """fp64: sum_m (logsumexp z_m - z_m[label_m]), and the gradient of UPSTREAM times that with respect to the logits"""
    z = x.astype(np.float64) + mask.astype(np.float64)[mask_row]
    zmax = z.max(axis=1, keepdims=True)
    e = np.exp(z - zmax)
    se = e.sum(axis=1, keepdims=True)
    rows = np.arange(len(labels))
    loss = float((zmax[:, 0] + np.log(se[:, 0]) - z[rows, labels]).sum())
    grad = e / se
    grad[rows, labels] -= 1.0
    return loss, UPSTREAM * grad


def bce_inputs(M):
    """logits +-100 in every combination with the labels 0 / 1"""
    i = np.arange(M)
    return np.where(i % 2 == 0, 100.0, -100.0).astype(np.float32), ((i // 2) % 2).astype(np.int64)


def bce_reference(s, y):
    s, y = s.astype(np.float64), y.astype(np.float64)
    loss = float((np.maximum(s, 0.0) - s * y + np.log1p(np.exp(-np.abs(s)))).sum())
    return loss, 1.0 / (1.0 + np.exp(-s)) - y


def within_bars(loss, grad, want_loss, want_grad, factor=1.0):
    """-> (loss ok, gradient ok, the two distances) under the bars divided by ``factor``"""
    dl, dg = abs(loss - want_loss), float(np.abs(np.asarray(grad, dtype=np.float64) - want_grad).max())
    return dl <= LOSS_RTOL / factor * max(abs(want_loss), 1.0), dg <= GRAD_ATOL / factor, dl, dg
