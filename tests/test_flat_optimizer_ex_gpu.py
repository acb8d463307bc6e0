"""GPU: the guarded / averaging Adam step and the flat exchange (ggpm_adam_step_ex, ggpm_flat_swap; csrc/gather.hip) through
``_lib``, and FlatAdam's guard, EMA and resumable state on the device.

The reference of every numeric check is torch in float64 on the CPU on the same fp32 inputs: ``clip_grad_norm_`` followed by
``torch.optim.Adam(param_groups)`` over separately allocated tensors, with ``optimizer.step()`` not called on the calls whose fp32
gradient norm is not finite, and the EMA recurrence in float64 with the decay rounded to fp32.  Bounds: parameters
``max|p - p64| <= 2e-6 max(1, max|p64|)`` after every step; the EMA after S applied steps
``2e-6 max(1, max|p64|) + 3 * 2^-24 * S * max(1, max|e64|)``.  Against ggpm_adam_step_groups (until a step has been skipped) and
across a resume the checks are equalities of bits.

Sizes: 64 (one tile, one workgroup), 64*7 (a zero padding tile at [128:192]) and one grid stride of the update kernel at its cap
plus 64*5 (a second grid-stride trip, and the 256-partial cap of the norm).

Measured (MI355X): see DESIGN 28.
"""
import ctypes
import io

import numpy as np
import pytest
import torch

from ggpm_amd import _lib, functional as F_
from test_flat_optimizer_gpu import (ADAM_STRIDE, ERR_ARG, HYPER, P_TOL, SENTINEL, _CountingLib, _Problem, _dev, _groups_c, _lib_,
                                     _partials, _reference_run, _step_groups, _tile_map)

pytestmark = pytest.mark.gpu

SIZES = [64, 64 * 7, ADAM_STRIDE + 64 * 5]
BAD_CALLS = (1, 4, 5)                # of 8, counted from 1: the first call, and two in a row
KIND = {1: "inf", 4: "nan", 5: "overflow"}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _step_ex(p, g, m, v, tiles_dev, groups, step, ws=None, count=0, max_norm=0.0, write_clipped=0, ema=None, decay=0.0,
             warmup=0, guard=0, ctr_in=None, ctr_out=None, status=None, n=None):
    return _lib_().ggpm_adam_step_ex(F_._p(p), F_._p(g), F_._p(m), F_._p(v), p.numel() if n is None else n, F_._p(tiles_dev),
                                     len(groups), ctypes.addressof(groups), step, F_._p(ws), count, max_norm, write_clipped,
                                     F_._p(ema), decay, warmup, guard, F_._p(ctr_in), F_._p(ctr_out), F_._p(status), F_._stream())


def _ema_bound(p64, e64, applied):
    return P_TOL * max(1.0, float(p64.abs().max())) + 3 * 2.0 ** -24 * applied * max(1.0, float(e64.abs().max()))


def _decay32(decay, warmup, t):
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + t) / np.float32(10 + t))
    return float(d)


_REF = {}


def _six_step_reference(prob, layout, mode):
    """_reference_run of the grouped-Adam tests (clip, torch.optim.Adam in float64, lr * 0.9 behind step 3), once per case."""
    key = (prob.n, layout, mode)
    if key not in _REF:
        n_groups, tiles = _tile_map(layout, prob.n // 64)
        max_norm = {"clipping": 0.5 * min(prob.norms), "not_clipping": 2.0 * max(prob.norms), "guard_only": None}[mode]
        _REF[key] = (max_norm, _reference_run(prob, n_groups, tiles, max_norm)[0])
    return _REF[key]


# ---------------------------------------------------------------------------------------------- through _lib: no skip yet
@pytest.mark.parametrize("mode", ["clipping", "not_clipping", "guard_only"])
@pytest.mark.parametrize("layout", ["one", "four"])
@pytest.mark.parametrize("n", SIZES)
def test_until_a_step_is_skipped_the_bits_are_those_of_adam_step_groups(n, layout, mode):
    """Six steps with the guard armed and nothing to refuse, on twin buffers: ggpm_adam_step_groups (guard_only: without
    partials), ggpm_adam_step_ex, and ggpm_adam_step_ex with an EMA (decay 0.999 under warm-up: the divided form)."""
    dev, lib = _dev(), _lib_()
    prob = _Problem.get(n)
    n_groups, tiles = _tile_map(layout, n // 64)
    max_norm, want = _six_step_reference(prob, layout, mode)
    tiles_dev = None if tiles is None else tiles.to(torch.uint8).to(dev)
    count = lib.ggpm_flat_sqnorm_workspace_bytes(n) // 8
    ws = torch.zeros(count, dtype=torch.float64, device=dev)
    runs = [[prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)] for _ in range(3)]
    ema = prob.p0.to(dev)
    e64 = prob.p0.double()
    ctr = torch.zeros(2, dtype=torch.int32, device=dev)
    status = torch.full((6,), SENTINEL, device=dev)
    clip_out = torch.zeros(2, device=dev)
    worst = 0.0
    for k, g_cpu in enumerate(prob.grads):
        g = g_cpu.to(dev)
        groups = _groups_c(HYPER[:n_groups], 0.9 if k >= 3 else 1.0)
        assert _partials(g, n, ws) == 0
        if max_norm is None:
            assert _step_groups(runs[0][0], g, runs[0][1], runs[0][2], tiles_dev, groups, k + 1) == 0
        else:
            assert _step_groups(runs[0][0], g, runs[0][1], runs[0][2], tiles_dev, groups, k + 1, ws, count, max_norm, clip_out) == 0
        cin, cout = ctr[k % 2:k % 2 + 1], ctr[1 - k % 2:2 - k % 2]
        for r, e in ((1, None), (2, ema)):
            assert _step_ex(runs[r][0], g, runs[r][1], runs[r][2], tiles_dev, groups, k + 1, ws, count, max_norm or 0.0, 0, e,
                            0.999, 1, 1, cin, cout, status) == 0
            for a, b in zip(runs[0], runs[r]):
                assert torch.equal(a, b), (k, r)
            st = status.cpu()
            assert float(st[2]) == 0.0 and float(st[3]) == k + 1 and bool((st[4:] == SENTINEL).all())
            assert abs(float(st[0]) - prob.norms[k]) <= 5e-7 * prob.norms[k]
            if max_norm is None:
                assert float(st[1]) == 1.0
            else:
                assert float(st[0]) == float(clip_out[0]) and float(st[1]) == float(clip_out[1])
        assert ctr.tolist() == [0, 0] and torch.equal(g.cpu(), g_cpu)
        e64 = e64 + (1.0 - _decay32(0.999, True, k + 1)) * (want[k] - e64)
        err, bound = float((ema.cpu().double() - e64).abs().max()), _ema_bound(want[k], e64, k + 1)
        worst = max(worst, err / bound)
        print("n=%d %s %s step %d: EMA err %.3e bound %.3e" % (n, layout, mode, k + 1, err, bound))
        assert err <= bound, (k, err, bound)
    if n >= 3 * 64:
        assert not bool(ema[128:192].any())


# ---------------------------------------------------------------------------------------------- through _lib: the guard
def _poison(g, kind, at):
    """One bad element at ``at``; 'overflow' keeps every element finite: two of 3e38 have a 2-norm of 4.2e38 > fp32's largest."""
    if kind == "overflow":
        g[at], g[at ^ 1] = 3e38, -3e38
    else:
        g[at] = float("inf") if kind == "inf" else float("nan")
    return g


_GUARD_REF = {}


def _guard_grads(prob):
    """Eight gradients: the six of the problem and two more at scales 0.2 and 1.5, none smaller than the smallest of the
    six, so that 0.5 * min(prob.norms) -- the clip of the grouped-Adam tests -- clips every call."""
    return prob.grads + [prob.grads[2] * 2.0, prob.grads[3] * 0.5]


def _guard_reference(prob, n_groups, tiles, max_norm, decay):
    """float64 on the CPU: per call the flat parameters and EMA, with clip_grad_norm_ + Adam.step() on the good calls only."""
    key = (prob.n, n_groups)
    if key in _GUARD_REF:
        return _GUARD_REF[key]
    idx = [torch.arange(prob.n)] if tiles is None else [
        (tiles.repeat_interleave(64) == k).nonzero().reshape(-1) for k in range(n_groups)]
    ps = [torch.nn.Parameter(prob.p0.double()[i].clone()) for i in idx]
    opt = torch.optim.Adam([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                            for q, h in zip(ps, HYPER)])
    e64, after, applied = prob.p0.double(), [], 0
    for call, g in enumerate(_guard_grads(prob), start=1):
        if call not in BAD_CALLS:
            for q, i in zip(ps, idx):
                q.grad = g.double()[i].clone()
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
            applied += 1
        flat = torch.empty(prob.n, dtype=torch.float64)
        for q, i in zip(ps, idx):
            flat[i] = q.detach()
        if call not in BAD_CALLS:
            e64 = e64 + (1.0 - _decay32(decay, False, applied)) * (flat - e64)
        after.append((flat, e64))
    _GUARD_REF[key] = after
    return after


@pytest.mark.parametrize("n,where", [(64, "first"), (64, "last"), (64 * 7, "first"), (64 * 7, "last"),
                                     (SIZES[2], "first"), (SIZES[2], "last"), (SIZES[2], "second_trip")])
def test_guard_sequence_of_eight_calls_against_float64(n, where):
    """Calls 1, 4 and 5 of 8 carry +Inf, a NaN, and a finite gradient whose norm overflows fp32; clipping on every call, with
    write_clipped, an EMA, and four groups where there are four tiles.  A kernel that took the host's call count for the bias
    corrections fails at call 2 (bc1 0.19 against 0.1)."""
    dev, lib = _dev(), _lib_()
    prob = _Problem.get(n)
    grads = _guard_grads(prob)
    n_groups, tiles = _tile_map("four" if n >= 4 * 64 else "one", n // 64)
    tiles_dev = None if tiles is None else tiles.to(torch.uint8).to(dev)
    max_norm, decay = 0.5 * min(prob.norms), 0.9
    want = _guard_reference(prob, n_groups, tiles, max_norm, decay)
    at = {"first": 0, "last": n - 1, "second_trip": ADAM_STRIDE + 7}[where]
    count = lib.ggpm_flat_sqnorm_workspace_bytes(n) // 8
    ws = torch.zeros(count, dtype=torch.float64, device=dev)
    p, m, v, ema = prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), prob.p0.to(dev)
    ctr = torch.zeros(2, dtype=torch.int32, device=dev)
    status = torch.full((6,), SENTINEL, device=dev)
    groups = _groups_c(HYPER[:n_groups])
    skipped = 0
    for call, g_cpu in enumerate(grads, start=1):
        bad = call in BAD_CALLS
        g_in = _poison(g_cpu.clone(), KIND[call], at) if bad else g_cpu
        if bad and KIND[call] == "overflow":
            assert bool(torch.isfinite(g_in).all())
        g = g_in.to(dev)
        before = [t.clone() for t in (p, m, v, ema, g)]
        cin, cout = (call - 1) % 2, call % 2
        assert _partials(g, n, ws) == 0
        assert _step_ex(p, g, m, v, tiles_dev, groups, call, ws, count, max_norm, 1, ema, decay, 0, 1, ctr[cin:cin + 1],
                        ctr[cout:cout + 1], status) == 0
        st = status.cpu()
        assert float(st[3]) == call - skipped and bool((st[4:] == SENTINEL).all())       # t_eff = step - *skipped_in
        if bad:
            skipped += 1
            assert float(st[2]) == 1.0 and not np.isfinite(float(st[0])), (call, st)
            for name, a, b in zip("pmveg", (p, m, v, ema, g), before):
                assert _same_bits(a, b), (call, name)
        else:
            assert float(st[2]) == 0.0 and float(st[1]) < 1.0 and np.isfinite(float(st[0]))
            assert torch.equal(g, before[4] * status[1])                                  # write_clipped: g * coef
        assert int(ctr[cout]) == skipped, (call, ctr.tolist())
        p64, e64 = want[call - 1]
        err, bound = float((p.cpu().double() - p64).abs().max()), P_TOL * max(1.0, float(p64.abs().max()))
        e_err, e_bound = float((ema.cpu().double() - e64).abs().max()), _ema_bound(p64, e64, call - skipped)
        print("n=%d %s call %d: err %.3e bound %.3e; EMA err %.3e bound %.3e" % (n, where, call, err, bound, e_err, e_bound))
        assert err <= bound and e_err <= e_bound, (call, err, bound, e_err, e_bound)
    assert skipped == 3
    if n >= 3 * 64:                                      # the padding tile is still zero in every stream
        assert not any(bool(t[128:192].any()) for t in (p, m, v, ema))


# ---------------------------------------------------------------------------------------------- through _lib: refusals, swap
def test_adam_step_ex_refuses_bad_arguments_and_writes_nothing():
    dev = _dev()
    n = 64 * 4
    bufs = [torch.full((n + 4,), SENTINEL, device=dev) for _ in range(5)]
    p, g, m, v, ema = (b[:n] for b in bufs)
    tiles = (torch.arange(n // 64) % 2).to(torch.uint8).to(dev)
    ws = torch.ones(4, dtype=torch.float64, device=dev)
    ctr = torch.full((3,), 7, dtype=torch.int32, device=dev)
    status = torch.full((4,), SENTINEL, device=dev)
    two = _groups_c(HYPER[:2])
    ok = dict(p=p, g=g, m=m, v=v, tiles_dev=tiles, groups=two, step=1, ws=ws, count=1, max_norm=1.0, write_clipped=1, ema=ema,
              decay=0.9, warmup=0, guard=1, ctr_in=ctr[0:1], ctr_out=ctr[1:2], status=status, n=n)

    def call(**kw):
        return _step_ex(**dict(ok, **kw))

    # what ggpm_adam_step_groups refuses
    for name, buf in zip("pgmv", bufs):
        assert call(**{name: buf[1:n + 1]}) == ERR_ARG
    assert call(n=0) == ERR_ARG and call(n=n - 4) == ERR_ARG and call(step=0) == ERR_ARG
    assert call(tiles_dev=None) == ERR_ARG and call(count=0) == ERR_ARG and call(count=257) == ERR_ARG
    for bad in (-1.0, float("nan")):
        assert call(max_norm=bad) == ERR_ARG
    # and what is new here
    assert call(ema=bufs[4][1:n + 1]) == ERR_ARG                                          # ema misaligned
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert call(decay=bad) == ERR_ARG                                                # ema_decay outside [0, 1)
    assert call(ws=None, count=0, max_norm=0.0) == ERR_ARG                               # the guard without partials
    assert call(ws=None, count=0, guard=0) == ERR_ARG                                    # a clip without partials
    assert call(ctr_out=ctr[0:1]) == ERR_ARG                                             # skipped_in == skipped_out
    assert call(ctr_in=None) == ERR_ARG and call(ctr_out=None) == ERR_ARG                # only one of the pair
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs) and bool((status == SENTINEL).all()) and ctr.tolist() == [7, 7, 7]


@pytest.mark.parametrize("n", SIZES + [67])
def test_flat_swap_is_an_exact_exchange_and_twice_is_the_identity(n):
    dev, lib = _dev(), _lib_()
    gen = torch.Generator().manual_seed(n)
    a_cpu, b_cpu = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    a_cpu[0], b_cpu[n - 1] = float("nan"), float("inf")                                  # bits, not values
    bufs = [torch.full((n + 8,), SENTINEL, device=dev) for _ in range(2)]
    a, b = bufs[0][4:4 + n], bufs[1][4:4 + n]
    a.copy_(a_cpu)
    b.copy_(b_cpu)
    assert lib.ggpm_flat_swap(F_._p(a), F_._p(b), n, F_._stream()) == 0
    assert _same_bits(a.cpu(), b_cpu) and _same_bits(b.cpu(), a_cpu)
    assert lib.ggpm_flat_swap(F_._p(a), F_._p(b), n, F_._stream()) == 0
    assert _same_bits(a.cpu(), a_cpu) and _same_bits(b.cpu(), b_cpu)
    for buf in bufs:
        assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all())
    s = F_._stream()
    assert lib.ggpm_flat_swap(None, F_._p(b), n, s) == ERR_ARG and lib.ggpm_flat_swap(F_._p(a), None, n, s) == ERR_ARG
    assert lib.ggpm_flat_swap(F_._p(a), F_._p(b), 0, s) == ERR_ARG and lib.ggpm_flat_swap(F_._p(a), F_._p(a), n, s) == ERR_ARG
    assert lib.ggpm_flat_swap(F_._p(bufs[0][5:]), F_._p(b), 1, s) == ERR_ARG               # misaligned
    assert _same_bits(a.cpu(), a_cpu) and _same_bits(b.cpu(), b_cpu)


# ---------------------------------------------------------------------------------------------- through FlatAdam
SHAPES = [(1,), (7,), (64,), (30, 62), (4096,), (63,), (65,), (1000,)]
GROUP_HYPER = [{"lr": 1e-2}, {"lr": 3e-3, "weight_decay": 0.01}, {"lr": 1e-3, "betas": (0.8, 0.99)}, {"lr": 2e-2, "eps": 1e-6}]


def _flat_adam(seed, grouped=True, **kw):
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(_dev())) for s in SHAPES]
    sync = FlatGradSync(params, keep_flat=True)
    if grouped:
        opt = FlatAdam(sync, param_groups=[dict(h, params=params[k::4]) for k, h in enumerate(GROUP_HYPER)], **kw)
    else:
        opt = FlatAdam(sync, lr=1e-2, **kw)
    return params, sync, opt


def _twins(params):
    twins = [torch.nn.Parameter(p.detach().cpu().double()) for p in params]
    return twins, torch.optim.Adam([dict(h, params=twins[k::4]) for k, h in enumerate(GROUP_HYPER)])


def _feed(params, sync, opt, call, bad=None):
    """Random gradients of call ``call`` (the same for every optimizer that asks), packed; ``bad`` poisons the packed buffer."""
    gen = torch.Generator().manual_seed(1000 + call)
    opt.zero_grad()
    grads = [torch.randn(p.shape, generator=gen) * (0.02 if call % 3 == 0 else 3.0) for p in params]
    for p, g in zip(params, grads):
        p.grad = g.to(p.device)
    sync.all_reduce()
    if bad is not None:
        _poison(sync.flat, bad, sync.offsets[4] + 11)
    return grads


def _check_against_twins(params, twins, opt, ema64, applied, tag):
    big = max(float(q.detach().abs().max()) for q in twins)
    err = max(float((p.detach().cpu().double() - q.detach()).abs().max()) for p, q in zip(params, twins))
    assert err <= P_TOL * max(1.0, big), (tag, err)
    if ema64 is None:
        return err, 0.0
    e_big = max(float(e.abs().max()) for e in ema64)
    e_err = max(float((g.cpu().double() - e).abs().max()) for g, e in zip(opt.ema_views, ema64))
    e_bound = P_TOL * max(1.0, big) + 3 * 2.0 ** -24 * applied * max(1.0, e_big)
    assert e_err <= e_bound, (tag, e_err, e_bound)
    return err, e_err / e_bound


@pytest.mark.parametrize("hip", [True, False])
def test_flat_adam_guard_and_ema_in_both_forms_against_float64(hip, monkeypatch):
    from ggpm_amd import _dev as dev_switches
    monkeypatch.setattr(dev_switches, "HIP_ADAM", hip)
    params, sync, opt = _flat_adam(7, skip_nonfinite=True, ema_decay=0.99, ema_warmup=True)
    assert opt._hip == hip and torch.equal(opt.ema, opt.flat.detach())
    twins, ref_opt = _twins(params)
    ema64 = [q.detach().clone() for q in twins]
    applied = 0
    for call in range(1, 9):
        bad = call in BAD_CALLS
        grads = _feed(params, sync, opt, call, KIND[call] if bad else None)
        before = [t.clone() for t in (opt.flat.detach(), opt.ema, sync.flat)]
        if not bad:
            for q, g in zip(twins, grads):
                q.grad = g.double()
            torch.nn.utils.clip_grad_norm_(twins, 20.0)
            ref_opt.step()
            applied += 1
            d = _decay32(0.99, True, applied)
            ema64 = [e + (1.0 - d) * (q.detach() - e) for e, q in zip(ema64, twins)]
        opt.step(clip_norm=20.0, write_clipped=True)
        assert opt.last_step_skipped.dim() == 0 and opt.last_step_skipped.is_cuda
        assert float(opt.last_step_skipped) == float(bad) and np.isfinite(float(opt.last_grad_norm)) == (not bad)
        if bad:
            assert all(_same_bits(a, b) for a, b in zip((opt.flat.detach(), opt.ema, sync.flat), before)), call
        err, e_frac = _check_against_twins(params, twins, opt, ema64, applied, call)
        print("hip=%s call %d: err %.3e; EMA error %.3f of its bound" % (hip, call, err, e_frac))
    assert opt.skipped_steps == 3 and opt.applied_steps == 5
    sd = opt.state_dict()
    assert sd["flat_adam"]["calls"] == 8 and sd["flat_adam"]["skipped"] == 3 and float(sd["state"][0]["step"]) == 5.0


def test_the_launches_of_a_step_with_the_features_off_and_on(monkeypatch):
    """Off: the entry points of today (ggpm_adam_step; partials + ggpm_adam_step_groups).  On: at most the partials and
    ggpm_adam_step_ex, with no host synchronisation."""
    def calls_of(opt, **kw):
        counting = _CountingLib(_lib.load())
        monkeypatch.setattr(_lib, "_LIB", counting)
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step(**kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.undo()
        return counting.calls

    params, sync, opt = _flat_adam(3, grouped=False)
    _feed(params, sync, opt, 1)
    assert calls_of(opt) == ["ggpm_adam_step"]
    assert calls_of(opt, clip_norm=20.0) == ["ggpm_flat_sqnorm_partials", "ggpm_adam_step_groups"]
    params, sync, opt = _flat_adam(3, grouped=True)
    _feed(params, sync, opt, 1)
    assert calls_of(opt) == ["ggpm_adam_step_groups"]
    assert not hasattr(opt, "_status") and opt.last_step_skipped is None
    for grouped in (False, True):
        for kw, clip, want in (({"skip_nonfinite": True}, None, ["ggpm_flat_sqnorm_partials", "ggpm_adam_step_ex"]),
                               ({"skip_nonfinite": True, "ema_decay": 0.9}, 20.0, ["ggpm_flat_sqnorm_partials", "ggpm_adam_step_ex"]),
                               ({"ema_decay": 0.9}, 20.0, ["ggpm_flat_sqnorm_partials", "ggpm_adam_step_ex"]),
                               ({"ema_decay": 0.9}, None, ["ggpm_adam_step_ex"])):
            params, sync, opt = _flat_adam(3, grouped=grouped, **kw)
            _feed(params, sync, opt, 1)
            assert calls_of(opt, clip_norm=clip) == want, (grouped, kw, clip)
            assert calls_of(opt, clip_norm=clip) == want
            assert opt.applied_steps == 2 and float(opt.last_step_skipped) == 0.0


def _through_file(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize("grouped", [False, True])
def test_resume_on_the_device_is_bit_equal_with_a_skipped_step_before_the_checkpoint(grouped):
    """Calls 1..3 with call 2 refused, checkpoint, calls 4..6; a fresh optimizer over other weights loads the checkpoint and
    takes calls 4..6: the dict has to carry calls (3) and skipped (1) apart for the bias corrections to agree."""
    kw = dict(skip_nonfinite=True, ema_decay=0.99, ema_warmup=True)
    params, sync, opt = _flat_adam(7, grouped, **kw)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt.opt, 0.9)
    for call in (1, 2, 3):
        _feed(params, sync, opt, call, "nan" if call == 2 else None)
        opt.step(clip_norm=20.0)
    sched.step()
    ckpt = _through_file({"params": [p.detach() for p in params], "opt": opt.state_dict(), "sched": sched.state_dict()})
    assert ckpt["opt"]["flat_adam"]["calls"] == 3 and ckpt["opt"]["flat_adam"]["skipped"] == 1
    assert float(ckpt["opt"]["state"][0]["step"]) == 2.0 and ckpt["opt"]["state"][3]["exp_avg"].shape == SHAPES[opt._order[3]]
    params2, sync2, opt2 = _flat_adam(8, grouped, **kw)
    sched2 = torch.optim.lr_scheduler.ExponentialLR(opt2.opt, 0.9)
    with torch.no_grad():
        for p, q in zip(params2, ckpt["params"]):
            p.copy_(q)
    opt2.load_state_dict(ckpt["opt"])
    sched2.load_state_dict(ckpt["sched"])
    assert opt2.skipped_steps == 1 and opt2.applied_steps == 2
    for o, ps, sy in ((opt, params, sync), (opt2, params2, sync2)):
        for call in (4, 5, 6):
            _feed(ps, sy, o, call, "inf" if call == 5 else None)
            o.step(clip_norm=20.0)
    assert opt.skipped_steps == opt2.skipped_steps == 2 and opt.applied_steps == opt2.applied_steps == 4
    for a, b in ((opt.flat.detach(), opt2.flat.detach()), (opt._m, opt2._m), (opt._v, opt2._v), (opt.ema, opt2.ema)):
        assert torch.equal(a, b)
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in opt2.param_groups]
    pad = torch.ones(opt2.flat.numel(), dtype=torch.bool, device=_dev())
    for p, off in zip(sync2.params, sync2.offsets):
        pad[off:off + p.numel()] = False
    assert not any(bool(t[pad].any()) for t in (opt2.flat.detach(), opt2._m, opt2._v, opt2.ema))


def test_a_dict_of_the_hip_form_loads_into_the_torch_op_form_and_continues(monkeypatch):
    from ggpm_amd import _dev as dev_switches
    kw = dict(skip_nonfinite=True, ema_decay=0.99)
    params, sync, opt = _flat_adam(7, True, **kw)
    twins, ref_opt = _twins(params)
    assert opt._hip

    def run(params, sync, opt, calls):
        for call in calls:
            bad = call in (2, 5)
            grads = _feed(params, sync, opt, call, "inf" if bad else None)
            if not bad:
                for q, g in zip(twins, grads):
                    q.grad = g.double()
                torch.nn.utils.clip_grad_norm_(twins, 20.0)
                ref_opt.step()
            opt.step(clip_norm=20.0)
            _check_against_twins(params, twins, opt, None, 0, call)

    run(params, sync, opt, (1, 2, 3))
    ckpt = _through_file({"params": [p.detach() for p in params], "opt": opt.state_dict()})
    monkeypatch.setattr(dev_switches, "HIP_ADAM", False)
    params2, sync2, opt2 = _flat_adam(8, True, **kw)
    assert not opt2._hip
    with torch.no_grad():
        for p, q in zip(params2, ckpt["params"]):
            p.copy_(q)
    opt2.load_state_dict(ckpt["opt"])
    assert opt2.skipped_steps == 1 and opt2.applied_steps == 2 and torch.equal(opt2.ema, opt.ema)
    run(params2, sync2, opt2, (4, 5, 6))
    assert opt2.skipped_steps == 2 and opt2.applied_steps == 4
    back = opt2.state_dict()                              # ... and the other direction: the torch-op form's dict into the HIP form
    monkeypatch.setattr(dev_switches, "HIP_ADAM", True)
    params3, sync3, opt3 = _flat_adam(9, True, **kw)
    with torch.no_grad():
        for p, q in zip(params3, params2):
            p.copy_(q)
    opt3.load_state_dict(back)
    assert opt3._hip and opt3.skipped_steps == 2 and opt3.applied_steps == 4
    run(params3, sync3, opt3, (7, 8))


def test_resume_on_a_real_model_is_bit_equal():
    """The smallest hierarchical golden batch, as test_gpu_training_loop.py builds it: two training steps, model and optimizer
    through torch.save / torch.load, two more; a freshly constructed model and optimizer load the checkpoint and take the
    same two.  The step is bitwise reproducible, so every parameter is equal."""
    from ggpm_amd.opvnet import OPVNet
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    from test_gpu_training_loop import _smallest_golden_case
    args, batch, schedule = _smallest_golden_case("hier-prop")

    def build(seed):
        torch.manual_seed(seed)
        model = OPVNet.get_model("hier-prop")(args).to(_dev())
        sync = FlatGradSync(model.parameters(), encoder=model.encoder, keep_flat=True)
        return model, sync, FlatAdam(sync, lr=1e-3, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)

    def steps(model, sync, opt, which):
        for i in which:
            torch.manual_seed(50 + i)                     # (the latent noise)
            opt.zero_grad()
            model(*batch, beta=0.3, perturb_z=True, schedule=schedule)[0].backward()
            sync.all_reduce()
            opt.step(clip_norm=20.0)

    model, sync, opt = build(5)
    assert opt._hip
    steps(model, sync, opt, (0, 1))
    ckpt = _through_file({"model": model.state_dict(), "opt": opt.state_dict()})
    steps(model, sync, opt, (2, 3))
    fresh, sync2, opt2 = build(6)
    fresh.load_state_dict(ckpt["model"])
    opt2.load_state_dict(ckpt["opt"])
    steps(fresh, sync2, opt2, (2, 3))
    assert opt.applied_steps == opt2.applied_steps == 4 and opt.skipped_steps == 0
    for (name, p), q in zip(model.named_parameters(), fresh.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(opt.ema, opt2.ema) and torch.equal(opt._m, opt2._m) and torch.equal(opt._v, opt2._v)
    with opt2.ema_weights():                              # the averaged weights evaluate, and differ from the trained ones
        torch.manual_seed(9)
        averaged = float(fresh(*batch, beta=0.3, perturb_z=True, schedule=schedule)[0])
    torch.manual_seed(9)
    assert np.isfinite(averaged) and averaged != float(fresh(*batch, beta=0.3, perturb_z=True, schedule=schedule)[0])
    assert torch.equal(opt.flat.detach(), opt2.flat.detach())
