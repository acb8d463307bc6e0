"""GPU: the attachment head (csrc/motif_assm.hip), the property heads and the latent search (csrc/property.hip) and the
small elementwise entry points, at the limits their entry points accept: every strided loop past its first trip, the
widths at and one past a tile, the dynamic-LDS and global-memory forms of the search, and the refusals just outside.
Every comparison is against an fp64 restatement that the CPU tests pin to the reference (motif_fixtures.
assm_head_reference, property_oracle.heads_step / search).  The conditions that make a comparison meaningful -- decision
margins, no ReLU unit at its kink -- are asserted on the fp64 side before the device result is looked at; the seeds were
chosen on the CPU so that they hold."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import property_oracle as po
from golden_utils import assert_close
from motif_fixtures import assm_head_reference, head_case
from property_fixtures import head_shapes, targets

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4


# ------------------------------------------------------------------------------------------ attachment head
UP = 1.5          # upstream factor of the loss


def _cycle_preds(P, C, mols):
    """P predictions (n, k, nth, b) cycling through singles and pairs, n == C (no pad row), n == 1 and nth 0 / 19; the
    molecule of prediction p is mols[p % len(mols)], so a molecule's predictions are interleaved with the others'."""
    kinds = [(2, 1, 3), (3, 2, 0), (C, 1, 19), (1, 2, 5), (C, 2, 7), (min(4, C), 1, 0)]
    return [kinds[p % 6] + (mols[p % len(mols)],) for p in range(P)]


_P6 = [(2, 1, 3, 0), (3, 2, 0, 2), (6, 1, 19, 1), (1, 2, 5, 0), (6, 2, 7, 2), (4, 1, 0, 1)]
HEAD_CASES = {
    # name: H, L, C, B, predictions; the seed is H + L, as in test_motif_vae_gpu.py
    "a_W256": (236, 24, 6, 3, _P6),            # W = H + 20 = 256: one full trip of bwd_w1's column loop
    "b_W257": (237, 24, 6, 3, _P6),            # one lane in its second trip
    "c_H257": (257, 56, 6, 3, _P6),            # second trip over H with one lane
    # one prediction: the only workgroup is also the last.  (n < C: with n == C and equal rows every score ties and the
    # gradients of z, W1, b1 and Wa are analytically zero -- nothing to compare a rounding with)
    "h_P1": (65, 24, 3, 1, [(2, 2, 19, 0)]),
    "f_L257": (24, 257, 6, 3, _P6),            # second trip over L in bwd_wa and bwd_z
    "i_P700": (65, 24, 6, 9, _cycle_preds(700, 6, list(range(9)))),       # arrival counter, in-order sum
    "d_H600": (600, 56, 9, 5, _cycle_preds(40, 9, [0, 1, 2, 4])),         # three trips; molecule 3 owns nothing
    "g_L1024": (24, 1024, 4, 2, [(4, 1, 0, 0), (1, 2, 19, 1), (2, 2, 5, 0), (3, 1, 0, 1)]),   # q reaches 3
    "e_H1004": (1004, 24, 4, 2, [(4, 1, 0, 0), (1, 2, 19, 1), (2, 2, 5, 0), (3, 1, 0, 1), (2, 1, 19, 1)]),
}
HEAD_ORDER = list(HEAD_CASES)      # (small shapes first, the tops of the envelope last)


def head_margin(scores, meta, distinct):
    """Smallest relative distance, over the predictions, between candidate 0's fp64 score and the largest other score,
    pad row included.  With equal rows the real candidates tie by construction (the restatement's tie rule covers
    them): only the pad row is a decision there."""
    worst = np.inf
    for p, (n, _k, _nth, _b, _coff, _roff) in enumerate(meta.tolist()):
        s = scores[p]
        others = s[1:] if distinct else s[n:]
        if others.size:
            o = others.max()
            worst = min(worst, abs(s[0] - o) / max(abs(s[0]), abs(o)))
    return worst


@functools.lru_cache(maxsize=None)
def head_reference(case, distinct):
    """-> (inputs, fp64 loss, accuracy, UP x the six gradients in the order rows, z, W1, b1, Wa, ba, decision margin)"""
    H, L, C, B, preds = HEAD_CASES[case]
    inp = head_case(H + L, H, L, C, preds, B, distinct)
    rows, meta, W1, b1, Wa, ba, z, _ = inp
    ref = [t.double().requires_grad_(True) for t in (rows, z, W1, b1, Wa, ba)]
    scores = []
    loss, acc = assm_head_reference(ref[0], meta, C, ref[2], ref[3], ref[4], ref[5], ref[1], scores_out=scores)
    (UP * loss).backward()
    return (inp, float(loss.detach()), float(acc), [r.grad.numpy() for r in ref],
            head_margin(scores[0].numpy(), meta, distinct))


def _head_leaves(inp, rows=None):
    r, _, W1, b1, Wa, ba, z, _ = inp
    return [r.to(DEV).requires_grad_(True) if rows is None else rows] + \
        [t.to(DEV).requires_grad_(True) for t in (z, W1, b1, Wa, ba)]


def _head_apply(inp, C, dv):
    from ggpm_amd.motif_decoder import _MotifAssm
    meta = inp[1]
    return _MotifAssm.apply(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], meta.to(DEV), meta.shape[0], C, inp[7])


HEAD_NAMES = ("rows", "z", "W1", "b1", "Wa", "ba")


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("case", HEAD_ORDER)
def test_head_kernel_at_the_accepted_limits(case, distinct):
    """Loss, accuracy and the six gradients against fp64 under an upstream factor of 1.5.  The accuracy is compared with
    ==: on the fp64 scores no decision is closer than 1e-4 of its magnitude."""
    H, L, C, B, preds = HEAD_CASES[case]
    inp, loss_r, acc_r, grads_r, margin = head_reference(case, distinct)
    assert margin > 1e-4, margin
    dv = _head_leaves(inp)
    loss, acc = _head_apply(inp, C, dv)
    (loss * UP).backward()
    loss_err = abs(float(loss.detach()) - loss_r) / max(1.0, abs(loss_r))
    print("%s distinct=%d margin %.2e loss err %.2e" % (case, distinct, margin, loss_err))
    fails = []
    for name, a, want in zip(HEAD_NAMES, dv, grads_r):
        got = a.grad.detach().cpu().double().numpy()
        scale = max(np.abs(want).max(), 1e-3)
        err = np.abs(got).max() if name == "ba" else np.abs(got - want).max() / scale
        print("   d%-4s %.2e" % (name, err))
        # ba: analytically zero (the softmax gradients of a prediction sum to 0): rounding noise only
        if err > (1e-5 if name == "ba" else TOL):
            fails.append((name, err))
    assert loss_err <= TOL
    assert float(acc) == acc_r
    assert not fails, fails
    used = set(p[3] for p in preds)
    for b in range(B):          # a molecule that owns no prediction: its dz row is exactly zero
        assert bool(dv[1].grad[b].ne(0).any()) == (b in used), b
    if case == "d_H600":
        assert 3 not in used


@pytest.mark.parametrize("H,L,P", [(1005, 8, 1), (8, 1025, 1), (8, 8, 0)])
def test_head_refuses_shapes_outside_the_envelope(H, L, P):
    """H + 20 > 1024, L > 1024 and no prediction at all: an error from the entry point's own check, nothing launched."""
    from ggpm_amd.motif_decoder import _MotifAssm
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    meta = torch.tensor([(1, 1, 0, 0, 0, 0)] * P, dtype=torch.int32, device=DEV).reshape(P, 6)
    with pytest.raises(RuntimeError, match="motif_assm_forward"):
        _MotifAssm.apply(z(1, H), z(1, L), z(H, H + 20), z(H), z(L, H), z(L), meta, P, 2, P)


def test_head_takes_rows_that_are_a_column_view_of_a_wider_buffer():
    """rows = buf[:, :H] of a [R, 264] buffer whose pad columns hold 7.0: loss and every gradient bitwise equal to the
    contiguous call, and rows.grad has the shape of rows."""
    case = "c_H257"
    H, L, C, B, _ = HEAD_CASES[case]
    inp = head_reference(case, True)[0]
    runs = []
    for strided in (False, True):
        rows = None
        if strided:
            buf = torch.full((inp[0].shape[0], 264), 7.0, device=DEV)
            buf[:, :H] = inp[0].to(DEV)
            rows = buf[:, :H].detach().requires_grad_(True)
            assert rows.stride() == (264, 1)
        dv = _head_leaves(inp, rows)
        loss, acc = _head_apply(inp, C, dv)
        (loss * UP).backward()
        assert dv[0].grad.shape == inp[0].shape
        runs.append([loss.detach(), acc.detach()] + [t.grad for t in dv])
        if strided:
            assert bool((buf[:, H:] == 7.0).all())
    for name, a, b in zip(("loss", "acc") + HEAD_NAMES, *runs):
        assert torch.equal(a, b), name


def test_head_twice_on_the_same_tensors_is_bitwise_equal():
    case = "d_H600"
    C = HEAD_CASES[case][2]
    inp = head_reference(case, True)[0]
    dv = _head_leaves(inp)
    runs = []
    for _ in range(2):
        loss, acc = _head_apply(inp, C, dv)
        runs.append([loss.detach(), acc.detach()] + list(torch.autograd.grad(loss * UP, dv)))
    for name, a, b in zip(("loss", "acc") + HEAD_NAMES, *runs):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------ property heads
HEADS_SEED = (12345, 678)
HEADS_CASES = [
    # B, half, hidden, extra latent columns, seed
    (5, 1, 1, 0, 102),                        # the smallest head the kernel accepts
    (20, 16, [64, 48, 40, 24], 3, 1100),       # z wider than 2 half: the extra columns' dz is exactly zero
    (1024, 12, [64, 64], 0, 2380),             # B at its bound: pl[] full, Dc initialised in two trips, 128 row chunks
    (600, 129, [257, 3], 0, 3163),             # widths one past a power of two, a narrow last hidden layer
    (37, 256, [512, 512], 0, 4128),            # every width at its bound: 8 trips of the output loop, the LDS ping-pong full
]


def _scaled_heads(half, hidden, dropout, seed):
    """PropertyOptimizer (CPU) with weights and biases of standard deviation 1 / sqrt(fan_in): predictions stay O(1) at
    width 512."""
    from ggpm_amd.property import PropertyOptimizer
    opt = PropertyOptimizer(half, hidden, dropout)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for head in (opt.homo_linear, opt.lumo_linear):
            for lin in head.linears():
                std = lin.in_features ** -0.5
                lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * std)
                lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen) * std)
    return opt


def _layers(opt, dtype=np.float64):
    sd = {k: v.detach().cpu().numpy() for k, v in opt.state_dict().items()}
    return po.head_layers(sd, "homo_linear", dtype), po.head_layers(sd, "lumo_linear", dtype)


def _min_preactivation(layers, x, masks, scale):
    _, acts = po.head_forward(layers, x, masks, scale)
    return min(float(np.abs(acts[i] @ W.T + b).min()) for i, (W, b) in enumerate(layers[:-1]))


@functools.lru_cache(maxsize=None)
def heads_reference(i, dropout):
    """-> (heads on the CPU, z, t_homo, t_lumo (fp32), property_oracle.heads_step in fp64, the smallest |hidden
    pre-activation| of that run)"""
    B, half, hidden, extra, seed = HEADS_CASES[i]
    opt = _scaled_heads(half, hidden, dropout, seed)
    rs = np.random.RandomState(seed + 1)
    z = rs.standard_normal((B, 2 * half + extra)).astype(np.float32)
    th, tl = rs.standard_normal(B).astype(np.float32), rs.standard_normal(B).astype(np.float32)
    homo, lumo = _layers(opt)
    z64 = z.astype(np.float64)
    ref = po.heads_step(homo, lumo, z64, half, th.astype(np.float64), tl.astype(np.float64), p=dropout, seed=HEADS_SEED,
                        dloss=(0.7, 1.3))
    scale = 1.0 / (1.0 - dropout) if dropout > 0 else 1.0
    kink = min(_min_preactivation(layers, z64[:, hi * half:(hi + 1) * half],
                                  po.heads_masks(B, layers, dropout, HEADS_SEED, site), scale)
               for hi, (layers, site) in enumerate(((homo, po.SITE_HOMO), (lumo, po.SITE_LUMO))))
    return opt, z, th, tl, ref, kink


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("i", range(len(HEADS_CASES)), ids=lambda i: "B%d_half%d" % HEADS_CASES[i][:2])
def test_property_heads_at_the_bounds_of_their_envelope(i, dropout):
    B, half, hidden, extra, _ = HEADS_CASES[i]
    opt, z, th, tl, ref, kink = heads_reference(i, dropout)
    # a unit that flips between fp32 and fp64 changes a gradient mask, not a rounding
    assert kink > 1e-5, kink
    opt = _scaled_heads(half, hidden, dropout, HEADS_CASES[i][4]).to(DEV)
    opt.train()
    opt._dropout_seed = HEADS_SEED
    z = torch.from_numpy(z).to(DEV).requires_grad_(True)
    lh, ll, ph, pl = opt.forward_latent(z, (torch.from_numpy(th).to(DEV), torch.from_numpy(tl).to(DEV)))
    (0.7 * lh + 1.3 * ll).backward()
    worst = [assert_close(ph.cpu().numpy(), ref["pred"][0], "homo pred"),
             assert_close(pl.cpu().numpy(), ref["pred"][1], "lumo pred")]
    assert abs(float(lh) - ref["loss"][0]) <= TOL * max(1.0, ref["loss"][0])
    assert abs(float(ll) - ref["loss"][1]) <= TOL * max(1.0, ref["loss"][1])
    worst.append(assert_close(z.grad.cpu().numpy(), ref["dz"], "dz"))
    assert not bool(z.grad[:, 2 * half:].ne(0).any())
    for hi, head in enumerate((opt.homo_linear, opt.lumo_linear)):
        for k, lin in enumerate(head.linears()):
            worst.append(assert_close(lin.weight.grad.cpu().numpy(), ref["grads"][hi][k][0], "dW %d.%d" % (hi, k)))
            worst.append(assert_close(lin.bias.grad.cpu().numpy(), ref["grads"][hi][k][1], "db %d.%d" % (hi, k)))
    print("heads B=%d half=%d %s p=%.1f: smallest |pre-activation| %.2e, worst norm-wise distance %.2e"
          % (B, half, hidden, dropout, kink, max(worst)))


@pytest.mark.parametrize("B,half", [(1025, 12), (4, 257)])
def test_property_heads_refuse_a_batch_or_an_input_width_past_the_envelope(B, half):
    opt = _scaled_heads(half, [8], 0.0, 0).to(DEV)
    z = torch.zeros(B, 2 * half, device=DEV)
    with pytest.raises(NotImplementedError):
        opt.forward_latent(z, (torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)))


# ------------------------------------------------------------------------------------------ latent search
SEARCH_B, SEARCH_STEPS, SEARCH_PATIENCE, SEARCH_THRESHOLD, SEARCH_DELTA, SEARCH_MAX_STEPS = 8, 20, 5.0, 0.1, 0.1, 10000
SEARCH_CASES = [
    # mode, latent, hidden, lr, seed, extra latent columns
    ("soft", 320, 40, 1.0, 300, 3),           # half = 160 > 128 lanes, weights in under 64 KiB of LDS
    ("fixed", 64, [96, 96], 1.0, 301, 0),     # ~102 KB of LDS: more than the default limit, weights resident
    ("soft", 64, [96, 96], 1.0, 302, 0),
    ("patience", 32, [256, 256], 1.0, 300, 0),    # ~560 KB of weights: read from global memory, hidden > 128 lanes
    ("fixed", 400, 130, 0.5, 306, 0),         # half = 200 > 128 lanes, weights in global memory
    ("patience", 512, [512], 1.0, 303, 0),    # half and hidden at their bounds
]


def _search_heads(latent, hidden, seed):
    from ggpm_amd.params import seeded_state_dict
    from ggpm_amd.property import PropertyOptimizer
    half = latent // 2
    sd = seeded_state_dict(head_shapes(half, hidden), seed, bias_scale=0.3)
    opt = PropertyOptimizer(half, hidden, 0.1)
    opt.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return opt.eval(), sd


@functools.lru_cache(maxsize=None)
def search_reference(i):
    """property_oracle.search in fp64 (with its decision margins) and in fp32 -> (z, t_homo, t_lumo, {dtype: (latent,
    predictions [2, B], steps, status)}, smallest margin)"""
    mode, latent, hidden, lr, seed, extra = SEARCH_CASES[i]
    half = latent // 2
    _, sd = _search_heads(latent, hidden, seed)
    homo, lumo = po.head_layers(sd, "homo_linear"), po.head_layers(sd, "lumo_linear")
    z = np.random.RandomState(seed + 1).standard_normal((SEARCH_B, latent + extra)).astype(np.float32)
    th, tl = targets(seed, SEARCH_B)
    runs, margins = {}, po.Margins()
    for dt in (np.float64, np.float32):
        zo, preds, n, st = po.search(mode, homo, lumo, z, half, th, tl, lr, SEARCH_STEPS, SEARCH_DELTA, SEARCH_PATIENCE,
                                     SEARCH_THRESHOLD, SEARCH_MAX_STEPS, dtype=dt,
                                     margins=margins if dt is np.float64 else None)
        runs[dt] = (zo.astype(np.float64), np.stack(preds).astype(np.float64), n, st)
    return z, th, tl, runs, margins.min


class _Args:
    def __init__(self, mode, lr):
        self.optimize_type, self.property_optim_step, self.patience = mode, SEARCH_STEPS, SEARCH_PATIENCE
        self.patience_threshold, self.property_delta, self.latent_lr = SEARCH_THRESHOLD, SEARCH_DELTA, lr
        self.max_steps = SEARCH_MAX_STEPS


class _Holder(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.property_optim = opt
        self.latent_size = opt.input_size


def _search_entry_point(opt, mode, z, th, tl, lr):
    """ggpm_property_latent_search on a latent wider than 2 half (the Python search always concatenates two halves)"""
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    from ggpm_amd.property_control import MODES
    B = z.shape[0]
    z_out = torch.full_like(z, 7.0)
    pred = torch.empty(2, B, dtype=torch.float32, device=z.device)
    steps = torch.empty(B, dtype=torch.int32, device=z.device)
    status = torch.empty(B, dtype=torch.int32, device=z.device)
    heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
    _lib.check(_lib.load().ggpm_property_latent_search(
        MODES[mode], B, F_._p(z), z.shape[1], opt.input_size, ctypes.byref(heads[0]), ctypes.byref(heads[1]), F_._p(th),
        F_._p(tl), lr, SEARCH_STEPS, SEARCH_DELTA, SEARCH_PATIENCE, SEARCH_THRESHOLD, SEARCH_MAX_STEPS, F_._p(z_out),
        F_._p(pred), F_._p(steps), F_._p(status), F_._stream()), "property_latent_search")
    return z_out, pred, steps, status


@pytest.mark.parametrize("i", range(len(SEARCH_CASES)),
                         ids=lambda i: "%s_latent%d" % SEARCH_CASES[i][:2])
def test_latent_search_beyond_resident_weights_and_128_lanes(i):
    """Step counts exactly, status, and final latents and predictions within max(1e-4, 4 x the restatement's own fp32
    distance to fp64) per element.  On the fp64 side first: every decision margin >= 1e-3, every row done, the final
    latent below 100 in magnitude, and the fp32 restatement takes the same number of steps."""
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    mode, latent, hidden, lr, seed, extra = SEARCH_CASES[i]
    half = latent // 2
    z, th, tl, runs, margin = search_reference(i)
    z64, p64, n64, st64 = runs[np.float64]
    z32, p32, n32, _ = runs[np.float32]
    assert margin >= 1e-3, margin
    assert (st64 == po.DONE).all()
    assert np.abs(z64).max() < 100.0, np.abs(z64).max()
    assert (n32 == n64).all(), (n32, n64)
    opt, _ = _search_heads(latent, hidden, seed)
    opt = opt.to(DEV)
    zz, tth, ttl = (torch.from_numpy(a).to(DEV) for a in (z, th, tl))
    if extra:
        out, pred, steps, status = _search_entry_point(opt, mode, zz, tth, ttl, lr)
        assert torch.equal(out[:, latent:], zz[:, latent:])
    else:
        search = HierPropertyVAEOptimizer(_Holder(opt), _Args(mode, lr))
        out = search._get_optimize_func()(zz[:, :half], zz[:, half:], tth, ttl)
        pred, steps, status = torch.stack(search.predictions), search.steps_taken, search.status
    out, pred = out.cpu().numpy().astype(np.float64), pred.cpu().numpy().astype(np.float64)
    bound, pbound = np.maximum(1e-4, 4 * np.abs(z32 - z64)), np.maximum(1e-4, 4 * np.abs(p32 - p64))
    err, perr = np.abs(out - z32), np.abs(pred - p32)
    print("search %s latent=%d %s lr=%g: margin %.2e, steps %s, |latent| <= %.1f, worst latent err %.2e (err / bound "
          "%.2f), worst prediction err %.2e (%.2f); distance to fp64 %.2e / %.2e"
          % (mode, latent, hidden, lr, margin, sorted(set(n64.tolist())), np.abs(z64).max(), err.max(),
             (err / bound).max(), perr.max(), (perr / pbound).max(), np.abs(out - z64).max(), np.abs(pred - p64).max()))
    assert (steps.cpu().numpy() == n64).all(), (steps.tolist(), n64.tolist())
    assert (status.cpu().numpy() == po.DONE).all()
    assert (err <= bound).all(), "latent: worst excess %.3e" % (err - bound).max()
    assert (perr <= pbound).all(), "predictions: worst excess %.3e" % (perr - pbound).max()


# ------------------------------------------------------------------------------------------ small entry points
def _call(name, *args):
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    _lib.check(getattr(_lib.load(), name)(*[F_._p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args],
                                          F_._stream()), name)


@pytest.mark.parametrize("zero_row0", [0, 1])
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "relu", "tanh", "sigmoid"])
@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 4), (37, 300, 304), (3, 257, 264), (2049, 62, 64)])
def test_act_backward_matches_numpy(rows, cols, ld, act, zero_row0):
    """dpre = dy * act'(y) from the activation's OUTPUT y; ReLU' is 0 at y == 0; row 0 zeroed on request; the pad columns
    of dpre are not written.  Bitwise where the formula is a select, 1e-6 of max(|formula|, |dy|) otherwise (one
    rounding of 1 - y^2 or y (1 - y), fused or not)."""
    from ggpm_amd import functional as F_
    assert (F_.ACT_NONE, F_.ACT_RELU, F_.ACT_TANH, F_.ACT_SIGMOID) == (0, 1, 2, 3)
    rs = np.random.RandomState(rows + cols + act)
    x = rs.standard_normal((rows, ld)).astype(np.float32)
    y = {0: x, 1: np.maximum(x, 0), 2: np.tanh(x), 3: 1 / (1 + np.exp(-x))}[act].astype(np.float32)
    if act == 1:
        y[rows // 2, 0] = 0.0                          # exactly at the kink
        y[-1, cols - 1] = -0.0
    dy = rs.standard_normal((rows, ld)).astype(np.float32)
    one = np.float32(1)
    want = {0: dy, 1: np.where(y > 0, dy, np.float32(0)), 2: dy * (one - y * y), 3: dy * y * (one - y)}[act].copy()
    if zero_row0:
        want[0] = 0
    dpre = torch.full((rows, ld), 7.0, device=DEV)
    _call("ggpm_act_backward", torch.from_numpy(dy).to(DEV), torch.from_numpy(y).to(DEV), rows, cols, ld, act, zero_row0,
          dpre)
    got = dpre.cpu().numpy()
    assert (got[:, cols:] == 7.0).all()
    if act < 2:
        assert np.array_equal(got[:, :cols], want[:, :cols])
    else:
        assert (np.abs(got - want)[:, :cols] <= 1e-6 * np.maximum(np.abs(want), np.abs(dy))[:, :cols]).all()
    if act == 1:
        assert got[rows // 2, 0] == 0 and got[-1, cols - 1] == 0


@pytest.mark.parametrize("M,N,ld", [(1, 1, 1), (5, 257, 264), (300, 2100, 2104)])
def test_scale_rows_is_an_fp32_multiply_of_the_first_n_columns(M, N, ld):
    rs = np.random.RandomState(M + N)
    d = rs.standard_normal((M, ld)).astype(np.float32)
    scale = np.float32(-1.7)
    t = torch.from_numpy(d).to(DEV)
    _call("ggpm_scale_rows", t, ld, M, N, torch.tensor([scale], device=DEV))
    got = t.cpu().numpy()
    assert np.array_equal(got[:, :N], d[:, :N] * scale)
    assert np.array_equal(got[:, N:], d[:, N:])


@pytest.mark.parametrize("rows,width", [(1, 1), (257, 5), (70000, 13)])
def test_extract_column_every_column(rows, width):
    from ggpm_amd import functional as F_
    mat = torch.from_numpy(np.random.RandomState(rows).randint(0, 2 ** 31 - 1, size=(rows, width)).astype(np.int64))
    dev = mat.to(DEV)
    for c in range(width):
        got = F_.extract_column(dev, c)
        assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), mat[:, c])


@pytest.mark.parametrize("with_eps", [True, False])
@pytest.mark.parametrize("B,L", [(1, 1), (37, 56)])
def test_rsample_entry_points_match_the_fp64_formula(B, L, with_eps):
    """ggpm_rsample_forward / _backward (B L = 2072: nine trips of the one workgroup's loop) against
    lv = -|pv|, kl = -0.5 sum(1 + lv - mean^2 - exp(lv)) / B, z = mean + exp(lv / 2) eps in fp64; eps null: z == mean."""
    rs = np.random.RandomState(B * L)
    mean, pv, eps, dz = (rs.standard_normal((B, L)).astype(np.float32) for _ in range(4))
    if B * L > 1:
        pv[0, 0] = 0.0                                  # d(-|p|)/dp is 0 at p == 0, as torch.abs
    dkl = np.float32(0.3)
    m, p, e, g = (a.astype(np.float64) for a in (mean, pv, eps, dz))
    if not with_eps:
        e = np.zeros_like(e)
    lv = -np.abs(p)
    kl_w = -0.5 * np.sum(1.0 + lv - m * m - np.exp(lv)) / B
    z_w = m + np.exp(lv / 2) * e
    dmean_w = g + dkl * m / B
    dlv = dkl * (-0.5 / B) * (1.0 - np.exp(lv)) + g * e * 0.5 * np.exp(lv / 2)
    dpv_w = -np.sign(p) * dlv
    t = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    mean_d, pv_d, eps_d, dz_d = t(mean), t(pv), (t(eps) if with_eps else None), t(dz)
    z_d, kl_d = torch.empty(B, L, device=DEV), torch.empty(1, device=DEV)
    dmean_d, dpv_d = torch.empty(B, L, device=DEV), torch.empty(B, L, device=DEV)
    _call("ggpm_rsample_forward", mean_d, pv_d, eps_d, B, L, z_d, kl_d)
    _call("ggpm_rsample_backward", mean_d, pv_d, eps_d, dz_d, torch.tensor([dkl], device=DEV), B, L, dmean_d, dpv_d)
    if not with_eps:
        assert torch.equal(z_d, mean_d)
    assert abs(float(kl_d) - kl_w) <= 2e-5 * max(abs(kl_w), 1e-6)
    for name, a, b in (("z", z_d, z_w), ("dmean", dmean_d, dmean_w), ("dpv", dpv_d, dpv_w)):
        assert np.abs(a.cpu().numpy() - b).max() <= 2e-5 * max(np.abs(b).max(), 1e-6), name
    if B * L > 1:
        assert float(dpv_d[0, 0]) == 0.0
