"""CPU: FlatAdam's resumable state, non-finite step guard and EMA weights (ggpm_amd/optim.py), on its torch-op form.

The reference of every numeric check is torch in float64 on the same fp32 inputs, as in test_flat_optimizer_cpu.py:
``clip_grad_norm_`` followed by ``torch.optim.Adam(param_groups)`` over separately allocated tensors, with ``optimizer.step()``
NOT called on the iterations whose fp32 gradient norm is not finite, and the EMA recurrence ``e += (1 - d)(p - e)`` run in
float64 with the decay rounded to fp32.  Bounds: parameters ``max|p - p64| <= 2e-6 max(1, max|p64|)`` after every step; the EMA
after S applied steps ``2e-6 max(1, max|p64|) + 3 * 2^-24 * S * max(1, max|e64|)`` (the parameter error enters with total weight
below 1; every step adds at most three fp32 roundings at the magnitude of e).  Resume checks are equalities of bits.
"""
import copy
import io

import numpy as np
import pytest
import torch

from ggpm_amd.optim import FlatAdam
from ggpm_amd.parallel import FlatGradSync
from test_flat_optimizer_cpu import P_TOL, _check_params, _data, _group_spec, _net, _reference

CLIP = 0.5                           # below some of this net's gradient norms and above others
BAD_CALLS = (1, 4, 5)                # of 8, counted from 1: the first call, and two in a row


def _build(model, grouped, **kw):
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    if grouped:
        opt = FlatAdam(sync, lr=1e-3, param_groups=[dict(hp, params=ps) for ps, hp in _group_spec(model)], **kw)
    else:
        opt = FlatAdam(sync, lr=1e-2, **kw)
    return sync, opt


def _spec(model, grouped):
    return _group_spec(model) if grouped else [(list(model.parameters()), {"lr": 1e-2})]


def _poison(sync, kind):
    """Make the packed gradient one the guard must refuse.  'overflow' keeps every element finite: two elements of 3e38
    have a 2-norm of 4.2e38, above fp32's largest 3.4e38."""
    flat = sync.flat
    if kind == "inf":
        flat[0] = float("inf")
    elif kind == "nan":
        flat[flat.numel() // 2] = float("nan")
    else:
        flat[1], flat[sync.offsets[-1]] = 3e38, 3e38
        assert bool(torch.isfinite(flat).all())


def _norm32(sync):
    """The fp32 gradient norm as the user sees it: accumulated in float64, rounded to fp32."""
    return torch.linalg.vector_norm(sync.flat.double()).to(torch.float32)


def _backward(model, sync, opt, i):
    opt.zero_grad()
    model(_data(i)).backward()
    sync.all_reduce()


def _snapshot(sync, opt):
    mv = opt._moments()
    moments = [] if mv is None else [t.clone() for t in mv[0] + mv[1]]
    return [opt.flat.detach().clone(), sync.flat.clone()] + ([opt.ema.clone()] if opt.ema is not None else []) + moments


def _bits_equal(a, b):
    """Equality of the bit patterns (a NaN in the gradient buffer equals itself)."""
    return len(a) == len(b) and all(x.dtype == y.dtype == torch.float32 and x.shape == y.shape
                                    and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
                                    for x, y in zip(a, b))


def _dicts_equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_dicts_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_dicts_equal(x, y) for x, y in zip(a, b))
    return a == b


def _through_file(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


# ---------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("variant", ["plain", "skipped_before", "scheduler"])
@pytest.mark.parametrize("grouped", [False, True])
def test_resumed_run_is_bit_equal_to_the_run_that_went_on(grouped, variant):
    """3 steps, checkpoint, 3 more; a fresh model and optimizer (other initial weights) load both dicts and take the same 3."""
    kw = dict(skip_nonfinite=True, ema_decay=0.99, ema_warmup=True)
    model = _net(seed=5)
    sync, opt = _build(model, grouped, **kw)
    assert opt.state_dict()["state"] == {} and opt.state_dict()["flat_adam"]["calls"] == 0
    sched = torch.optim.lr_scheduler.ExponentialLR(opt.opt, 0.9) if variant == "scheduler" else None

    def run(model, sync, opt, sched, steps):
        for i in steps:
            _backward(model, sync, opt, i)
            if variant == "skipped_before" and i == 1:
                _poison(sync, "inf")
            opt.step(clip_norm=CLIP)
            if sched is not None and i in (1, 4):
                sched.step()

    run(model, sync, opt, sched, range(3))
    ckpt = _through_file({"model": model.state_dict(), "opt": opt.state_dict(),
                          "sched": sched.state_dict() if sched is not None else None})
    want_skipped = 1 if variant == "skipped_before" else 0
    assert ckpt["opt"]["flat_adam"]["calls"] == 3 and ckpt["opt"]["flat_adam"]["skipped"] == want_skipped
    assert float(ckpt["opt"]["state"][0]["step"]) == 3 - want_skipped
    run(model, sync, opt, sched, range(3, 6))

    fresh = _net(seed=99)
    sync2, opt2 = _build(fresh, grouped, **kw)
    sched2 = torch.optim.lr_scheduler.ExponentialLR(opt2.opt, 0.9) if sched is not None else None
    fresh.load_state_dict(ckpt["model"])
    opt2.load_state_dict(ckpt["opt"])
    assert _dicts_equal(opt2.state_dict(), ckpt["opt"])
    if sched2 is not None:
        sched2.load_state_dict(ckpt["sched"])
        assert [g["lr"] for g in opt2.param_groups] == pytest.approx([0.9 * hp["lr"] for _, hp in _spec(fresh, grouped)])
        assert all("initial_lr" in g for g in opt2.param_groups)
    assert all(p.data_ptr() == opt2.flat.data_ptr() + 4 * off for p, off in zip(sync2.params, sync2.offsets))
    run(fresh, sync2, opt2, sched2, range(3, 6))

    assert opt2.skipped_steps == opt.skipped_steps == want_skipped and opt2.applied_steps == opt.applied_steps == 6 - want_skipped
    assert torch.equal(opt.flat, opt2.flat) and torch.equal(opt.ema, opt2.ema)
    for a, b in zip(opt._moments(), opt2._moments()):
        assert _bits_equal(a, b)
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in opt2.param_groups]
    assert _dicts_equal(opt.state_dict(), opt2.state_dict())
    pad = torch.ones(opt2.flat.numel(), dtype=torch.bool)
    for p, off in zip(sync2.params, sync2.offsets):
        pad[off:off + p.numel()] = False
    if not grouped:                                      # the flat moments of the one anonymous tensor: padding stayed zero
        st = opt2.opt.state[opt2.flat]
        assert not bool(st["exp_avg"][pad].any()) and not bool(st["exp_avg_sq"][pad].any())
    assert not bool(opt2.ema[pad].any()) and not bool(opt2.flat.detach()[pad].any())


# ---------------------------------------------------------------------------------------------- interop with torch
def test_a_torch_adam_checkpoint_is_taken_over_and_continues_within_the_bound():
    a = _net(seed=4)
    topt = torch.optim.Adam(a.parameters(), lr=1e-2)
    for i in range(3):
        topt.zero_grad()
        a(_data(i)).backward()
        topt.step()
    sd = _through_file(topt.state_dict())
    b = _net(seed=17)
    b.load_state_dict(a.state_dict())
    sync, opt = _build(b, grouped=False)
    opt.load_state_dict(sd)
    assert opt.applied_steps == 3 and opt.skipped_steps == 0 and opt.state_dict()["flat_adam"]["calls"] == 3
    twin, ref_opt = _reference(b, _spec(b, False))           # torch continuing in float64 from the same checkpoint
    ref_opt.load_state_dict(sd)
    assert all(ref_opt.state[q]["exp_avg"].dtype == torch.float64 for q in twin.values())
    for i in range(3, 6):
        _backward(b, sync, opt, i)
        for p in b.parameters():
            twin[id(p)].grad = p.grad.detach().double().clone()
        ref_opt.step()
        opt.step()
        _check_params(b, twin, i)
    assert opt.applied_steps == 6


@pytest.mark.parametrize("grouped", [False, True])
def test_torch_adam_loads_a_flat_adam_state_dict(grouped):
    model = _net(seed=8)
    sync, opt = _build(model, grouped, ema_decay=0.9)
    for i in range(3):
        _backward(model, sync, opt, i)
        opt.step(clip_norm=CLIP)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "flat_adam"}            # torch ignores the extra top-level key
    order = [p for ps, _ in _spec(model, grouped) for p in ps]
    assert [i for g in sd["param_groups"] for i in g["params"]] == list(range(len(order)))
    if grouped:
        topt = torch.optim.Adam([{"params": ps} for ps, _ in _spec(model, True)])
    else:
        topt = torch.optim.Adam(list(sync.params))
    topt.load_state_dict(sd)
    want_m, want_v = opt._moments()
    slot = {id(p): i for i, p in enumerate(sync.params)}
    for j, p in enumerate(order):
        st = topt.state[p]
        assert float(st["step"]) == 3.0 and st["exp_avg"].shape == p.shape
        assert torch.equal(st["exp_avg"], want_m[slot[id(p)]]) and torch.equal(st["exp_avg_sq"], want_v[slot[id(p)]])
        assert torch.equal(sd["state"][j]["exp_avg"], st["exp_avg"])
    for g, (_, hp) in zip(topt.param_groups, _spec(model, grouped)):
        assert g["lr"] == hp["lr"] and g["betas"] == hp.get("betas", (0.9, 0.999))


# ---------------------------------------------------------------------------------------------- refusals
def test_load_state_dict_refuses_what_the_issue_lists_and_changes_nothing():
    model = _net(seed=2)
    sync, opt = _build(model, grouped=True, skip_nonfinite=True)
    for i in range(2):
        _backward(model, sync, opt, i)
        opt.step()
    good = opt.state_dict()
    before, lrs = _snapshot(sync, opt), [dict((k, v) for k, v in g.items() if k != "params") for g in opt.param_groups]

    def refused(sd, match):
        with pytest.raises(ValueError, match=match):
            opt.load_state_dict(sd)
        assert _bits_equal(_snapshot(sync, opt), before) and _dicts_equal(opt.state_dict(), good)
        assert [dict((k, v) for k, v in g.items() if k != "params") for g in opt.param_groups] == lrs

    bad = copy.deepcopy(good)                            # another number of groups
    bad["param_groups"] = bad["param_groups"][:3]
    refused(bad, "3 parameter group")
    bad = copy.deepcopy(good)                            # another number of parameters in group 1
    bad["param_groups"][1]["params"].append(99)
    bad["param_groups"][1]["lr"] = 123.0
    refused(bad, "group 1 holds 3")
    bad = copy.deepcopy(good)                            # a shape
    bad["state"][2]["exp_avg_sq"] = torch.zeros(5, 7)
    refused(bad, "exp_avg_sq of parameter 2")
    bad = copy.deepcopy(good)                            # one parameter at another step
    bad["state"][3]["step"] = torch.tensor(5.0)
    refused(bad, "parameter 3 is at step 5")
    bad = copy.deepcopy(good)                            # one parameter without state
    del bad["state"][1]
    refused(bad, "parameter 1 is at step 0")
    bad = copy.deepcopy(good)                            # an EMA, and this optimizer averages nothing
    bad["flat_adam"]["ema"] = {j: torch.zeros_like(p) for j, p in enumerate(sync.params)}
    refused(bad, "EMA")
    opt.load_state_dict(good)                            # and the good one still loads
    assert _bits_equal(_snapshot(sync, opt), before)
    # the constructor's own refusals
    s2 = FlatGradSync(_net(seed=2).parameters(), keep_flat=True)
    for kw in ({"ema_decay": 1.0}, {"ema_decay": -0.1}, {"ema_warmup": True}):
        with pytest.raises(ValueError, match="ema"):
            FlatAdam(s2, **kw)


# ---------------------------------------------------------------------------------------------- guard and EMA
def _ema_bound(p64_max, e64_max, applied):
    return P_TOL * max(1.0, p64_max) + 3 * 2.0 ** -24 * applied * max(1.0, e64_max)


def _decay32(decay, warmup, t):
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + t) / np.float32(10 + t))
    return float(d)


def _check_ema(model, opt, twin, ema64, applied, tag):
    slot = {id(p): i for i, p in enumerate(opt.sync.params)}
    worst = 0.0
    for p in model.parameters():
        e64, got = ema64[id(p)], opt.ema_views[slot[id(p)]].double()
        err = float((got - e64).abs().max())
        bound = _ema_bound(float(twin[id(p)].detach().abs().max()), float(e64.abs().max()), applied)
        worst = max(worst, err / bound)
        assert err <= bound, (tag, tuple(p.shape), err, bound)
    return worst


@pytest.mark.parametrize("kind", ["inf", "nan", "overflow"])
@pytest.mark.parametrize("grouped", [False, True])
def test_guard_skips_calls_1_4_5_of_8_and_matches_torch_not_stepping(grouped, kind):
    model = _net(seed=5)
    twin, ref_opt = _reference(model, _spec(model, grouped))
    sync, opt = _build(model, grouped, skip_nonfinite=True, ema_decay=0.9)
    ema64 = {id(p): p.detach().double().clone() for p in model.parameters()}
    applied = 0
    for call in range(1, 9):
        _backward(model, sync, opt, call)
        if call in BAD_CALLS:
            _poison(sync, kind)
        norm32 = _norm32(sync)
        assert bool(torch.isfinite(norm32)) == (call not in BAD_CALLS)
        before = _snapshot(sync, opt)
        if call not in BAD_CALLS:                        # the oracle: clip and step only where the fp32 norm is finite
            for p in model.parameters():
                twin[id(p)].grad = p.grad.detach().double().clone()
            torch.nn.utils.clip_grad_norm_(list(twin.values()), CLIP)
            ref_opt.step()
            applied += 1
            for p in model.parameters():
                e = ema64[id(p)]
                e += (1.0 - _decay32(0.9, False, applied)) * (twin[id(p)].detach() - e)
        opt.step(clip_norm=CLIP)
        assert float(opt.last_step_skipped) == float(call in BAD_CALLS) and opt.last_step_skipped.dim() == 0
        if call in BAD_CALLS:
            assert _bits_equal(_snapshot(sync, opt), before), call
            assert not bool(torch.isfinite(opt.last_grad_norm))
        else:
            assert float(opt.last_grad_norm) == float(norm32)
        assert opt.applied_steps == applied and opt.skipped_steps == call - applied
        _check_params(model, twin, call)
        worst = _check_ema(model, opt, twin, ema64, applied, call)
    print("grouped=%s %s: EMA error at most %.3f of its bound after %d applied steps" % (grouped, kind, worst, applied))
    assert opt.skipped_steps == 3 and opt.applied_steps == 5
    assert opt.state_dict()["flat_adam"]["calls"] == 8 and float(opt.state_dict()["state"][0]["step"]) == 5.0


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("grouped", [False, True])
def test_ema_follows_the_float64_recurrence(grouped, decay, warmup):
    model = _net(seed=6)
    twin, ref_opt = _reference(model, _spec(model, grouped))
    sync, opt = _build(model, grouped, ema_decay=decay, ema_warmup=warmup)
    assert opt.ema_decay == float(np.float32(decay)) and torch.equal(opt.ema, opt.flat.detach())
    assert all(torch.equal(e, p.detach()) and e.shape == p.shape for e, p in zip(opt.ema_views, sync.params))
    ema64 = {id(p): p.detach().double().clone() for p in model.parameters()}
    worst = 0.0
    for step in range(1, 9):
        _backward(model, sync, opt, step)
        for p in model.parameters():
            twin[id(p)].grad = p.grad.detach().double().clone()
        ref_opt.step()
        opt.step()
        d = _decay32(decay, warmup, step)
        for p in model.parameters():
            e = ema64[id(p)]
            e += (1.0 - d) * (twin[id(p)].detach() - e)
        _check_params(model, twin, step)
        worst = max(worst, _check_ema(model, opt, twin, ema64, step, step))
    print("grouped=%s decay=%g warmup=%s: EMA error at most %.3f of its bound" % (grouped, decay, warmup, worst))
    assert not torch.equal(opt.ema, opt.flat.detach())


@pytest.mark.parametrize("grouped", [False, True])
def test_ema_weights_swaps_in_and_restores_also_when_the_body_raises(grouped):
    model = _net(seed=7)
    sync, opt = _build(model, grouped, ema_decay=0.9)
    for i in range(3):
        _backward(model, sync, opt, i)
        opt.step()
    trained, averaged = opt.flat.detach().clone(), opt.ema.clone()
    avg_views = [e.clone() for e in opt.ema_views]
    slot = {id(p): i for i, p in enumerate(sync.params)}
    ptrs = [p.data_ptr() for p in sync.params]
    assert not torch.equal(trained, averaged)
    with opt.ema_weights():
        sd = model.state_dict()
        for name, p in model.named_parameters():
            assert torch.equal(sd[name], avg_views[slot[id(p)]]), name
        assert torch.equal(sd["out.weight"], avg_views[slot[id(model.emb.weight)]])      # the tied weight too
        assert torch.equal(opt.ema, trained)
        inside = float(model(_data(0)).detach())
    assert torch.equal(opt.flat.detach(), trained) and torch.equal(opt.ema, averaged)
    assert inside != float(model(_data(0)).detach())
    with pytest.raises(RuntimeError, match="boom"):
        with opt.ema_weights():
            assert torch.equal(opt.flat.detach(), averaged)
            raise RuntimeError("boom")
    assert torch.equal(opt.flat.detach(), trained) and torch.equal(opt.ema, averaged)
    assert [p.data_ptr() for p in sync.params] == ptrs
    plain = FlatAdam(FlatGradSync(_net(seed=7).parameters(), keep_flat=True))
    assert plain.ema is None and plain.ema_views is None and not plain.skip_nonfinite
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.reset_ema()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass
