"""CPU: at the large logits of tests/loss_extreme_cases.py torch's own fp32 losses stay inside the GPU test's bars (2e-5
relative on the loss, 2e-6 absolute on the gradient, against numpy fp64) with a factor of two to spare, so those bars ask
of the HIP kernels nothing that fp32 arithmetic cannot deliver."""
import pytest
import torch

import loss_extreme_cases as L


@pytest.mark.parametrize("M,N", L.SHAPES)
def test_torch_fp32_softmax_ce_is_within_half_the_bars(M, N):
    x, labels, mask, mask_row = L.ce_inputs(M, N)
    assert (mask == L.MASK_VALUE).any() and abs(x).max() > 80
    z = torch.from_numpy(x).requires_grad_(True)
    zz = z + torch.from_numpy(mask)[torch.from_numpy(mask_row)]
    loss = torch.nn.functional.cross_entropy(zz, torch.from_numpy(labels), reduction="sum")
    (L.UPSTREAM * loss).backward()
    ok_l, ok_g, dl, dg = L.within_bars(float(loss.detach()), z.grad.numpy(), *L.ce_reference(x, labels, mask, mask_row), factor=2.0)
    print("torch fp32 softmax CE (%d, %d): loss off by %.2e of %.4g, gradient by %.2e" % (M, N, dl, float(loss.detach()), dg))
    assert ok_l and ok_g


def test_torch_fp32_bce_is_within_half_the_bars():
    s, y = L.bce_inputs(257)
    t = torch.from_numpy(s).requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(t, torch.from_numpy(y).float(), reduction="sum")
    loss.backward()
    ok_l, ok_g, dl, dg = L.within_bars(float(loss.detach()), t.grad.numpy(), *L.bce_reference(s, y), factor=2.0)
    print("torch fp32 BCE at +-100: loss off by %.2e of %.4g, gradient by %.2e" % (dl, float(loss.detach()), dg))
    assert ok_l and ok_g
