"""CPU: FlatAdam with parameter groups and gradient-norm clipping (ggpm_amd/optim.py), on its torch-op form.

The reference of every numeric check is torch in float64 on the same fp32 inputs: ``clip_grad_norm_`` followed by
``torch.optim.Adam`` with ``param_groups`` over separately allocated per-parameter tensors, fed the fp32 gradients of the model
under test.  Bounds: parameters ``max|p - p64| <= 2e-6 max(1, max|p64|)`` after every step (the bar of
test_adam_step_matches_torch_adam); norms ``<= 5e-7`` relative (fp64 accumulation and one rounding through sqrt to fp32 are at
most two fp32 roundings, 1.2e-7; the bound leaves four ulps).
"""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ggpm_amd.optim import FlatAdam
from ggpm_amd.parallel import FlatGradSync, broadcast_parameters

P_TOL, NORM_TOL = 2e-6, 5e-7
CLIP_LOW, CLIP_HIGH = 1e-3, 1e3         # below / above every step's gradient norm (asserted on the reference side)


class Net(torch.nn.Module):
    """An embedding tied to the output projection, and a head that ends in a bias of ONE float."""

    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(11, 6)
        self.body = torch.nn.Linear(6, 5)
        self.head = torch.nn.Linear(5, 1)
        self.out = torch.nn.Linear(6, 11, bias=False)
        self.out.weight = self.emb.weight

    def forward(self, idx):
        h = self.emb(idx)
        return self.head(torch.tanh(self.body(h))).pow(2).mean() + self.out(h).logsumexp(-1).mean()


def _net(seed):
    torch.manual_seed(seed)
    return Net()


def _data(i):
    g = torch.Generator().manual_seed(100 + i)
    return torch.randint(0, 11, (7,), generator=g)


def _group_spec(model):
    """Four groups by name, as vae_fine_tune_indv_opt.py splits its model: (name test, hyper-parameters)."""
    named = list(model.named_parameters())            # the tied weight appears once, as emb.weight
    pick = lambda key: [p for n, p in named if n.startswith(key)]
    return [(pick("emb"), {"lr": 1e-2}), (pick("body"), {"lr": 3e-3, "weight_decay": 0.01}),
            (pick("head.weight"), {"lr": 1e-3, "betas": (0.8, 0.99)}), (pick("head.bias"), {"lr": 2e-2, "eps": 1e-6})]


def _reference(model, spec):
    """fp64 copies of the parameters in separately allocated tensors, and torch.optim.Adam over the same groups."""
    twin = {id(p): torch.nn.Parameter(p.detach().double().clone()) for p in model.parameters()}
    groups = [dict(hp, params=[twin[id(p)] for p in ps]) for ps, hp in spec]
    return twin, torch.optim.Adam(groups, lr=1e-3)


def _check_params(model, twin, step):
    for p in model.parameters():
        q = twin[id(p)].detach()
        err = float((p.detach().double() - q).abs().max())
        assert err <= P_TOL * max(1.0, float(q.abs().max())), (step, tuple(p.shape), err)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("clip_norm", [CLIP_LOW, CLIP_HIGH])
def test_clipped_steps_match_torch_in_float64(clip_norm, grouped):
    """Six steps of step(clip_norm=...) with an ExponentialLR step in the middle: four groups, and the default single group."""
    model = _net(seed=5)
    spec = _group_spec(model) if grouped else [(list(model.parameters()), {"lr": 1e-2})]
    twin, ref_opt = _reference(model, spec)
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    opt = (FlatAdam(sync, lr=1e-3, param_groups=[dict(hp, params=ps) for ps, hp in spec]) if grouped
           else FlatAdam(sync, lr=1e-2))
    assert len(opt.param_groups) == len(spec) and opt.param_groups is opt.opt.param_groups
    sched, ref_sched = (torch.optim.lr_scheduler.ExponentialLR(o, 0.9) for o in (opt.opt, ref_opt))
    for step in range(6):
        opt.zero_grad()
        model(_data(step)).backward()
        sync.all_reduce()
        for p in model.parameters():
            twin[id(p)].grad = p.grad.detach().double().clone()
        # the norms the training scripts print, before the step touches anything
        want_g = math.sqrt(sum(float(q.grad.norm()) ** 2 for q in twin.values()))
        want_p = math.sqrt(sum(float(p.detach().double().norm()) ** 2 for p in model.parameters()))
        assert abs(float(opt.grad_norm()) - want_g) <= NORM_TOL * want_g
        assert abs(float(opt.param_norm()) - want_p) <= NORM_TOL * want_p
        assert opt.grad_norm().dim() == 0 and opt.param_norm().dim() == 0
        ref_norm = float(torch.nn.utils.clip_grad_norm_(list(twin.values()), clip_norm))
        assert (ref_norm > clip_norm) if clip_norm == CLIP_LOW else (ref_norm < clip_norm), (step, ref_norm)
        ref_opt.step()
        opt.step(clip_norm=clip_norm)
        assert opt.last_grad_norm.dim() == 0 and opt.last_clip_coef.dim() == 0
        assert abs(float(opt.last_grad_norm) - ref_norm) <= NORM_TOL * ref_norm, (step, float(opt.last_grad_norm), ref_norm)
        want_coef = min(clip_norm / (ref_norm + 1e-6), 1.0)
        assert abs(float(opt.last_clip_coef) - want_coef) <= 2 * NORM_TOL * want_coef
        _check_params(model, twin, step)
        if step == 2:
            sched.step()
            ref_sched.step()
            assert [g["lr"] for g in opt.param_groups] == pytest.approx([0.9 * hp["lr"] for _, hp in spec])
    assert all(p.data_ptr() == opt.flat.data_ptr() + 4 * off for p, off in zip(sync.params, sync.offsets))


def test_grouped_steps_without_a_clip_match_torch_in_float64():
    model = _net(seed=6)
    spec = _group_spec(model)
    twin, ref_opt = _reference(model, spec)
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    opt = FlatAdam(sync, lr=1e-3, param_groups=[dict(hp, params=ps) for ps, hp in spec])
    for step in range(6):
        opt.zero_grad()
        model(_data(step)).backward()
        sync.all_reduce()
        for p in model.parameters():
            twin[id(p)].grad = p.grad.detach().double().clone()
        ref_opt.step()
        opt.step()
        _check_params(model, twin, step)
    assert opt.last_grad_norm is None


def test_default_flat_adam_still_equals_adam_over_the_parameter_list():
    """No groups, no clip: exactly torch.optim.Adam's parameters, as test_flat_adam_equals_adam_over_the_parameter_list demands."""
    a, b = _net(seed=3), _net(seed=3)
    oa = torch.optim.Adam(a.parameters(), lr=1e-2)
    sync = FlatGradSync(b.parameters(), keep_flat=True)
    ob = FlatAdam(sync, lr=1e-2)
    assert len(ob.param_groups) == 1
    for i in range(4):
        oa.zero_grad()
        a(_data(i)).backward()
        oa.step()
        ob.zero_grad()
        b(_data(i)).backward()
        sync.all_reduce()
        ob.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_construction_and_step_refuse_what_the_issue_lists():
    model = _net(seed=1)
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    ps = list(model.parameters())
    before = [p.data_ptr() for p in ps]
    stranger = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="in groups 0 and 1"):
        FlatAdam(sync, param_groups=[{"params": ps}, {"params": ps[:1]}])
    with pytest.raises(ValueError, match="in no group"):
        FlatAdam(sync, param_groups=[{"params": ps[:-1]}])
    with pytest.raises(ValueError, match="not in the FlatGradSync"):
        FlatAdam(sync, param_groups=[{"params": ps}, {"params": [stranger]}])
    with pytest.raises(ValueError, match="1 to 8"):
        FlatAdam(sync, param_groups=[{"params": [p]} for p in ps] + [{"params": []} for _ in range(9 - len(ps))])
    assert [p.data_ptr() for p in ps] == before           # a refused construction re-pointed nothing
    # a tied parameter reached twice within ONE group counts once; eight groups are accepted
    opt = FlatAdam(sync, param_groups=[{"params": ps + [model.out.weight, model.emb.weight]}])
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == len(ps)
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_norm"):
            opt.step(clip_norm=bad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _net(seed=rank)
    broadcast_parameters(model, src=0)
    sync = FlatGradSync(model.parameters())
    opt = FlatAdam(sync, lr=1e-3, param_groups=[dict(hp, params=ps) for ps, hp in _group_spec(model)])
    norms = []
    for step in range(3):
        opt.zero_grad()
        model(_data(2 * step + rank)).backward()          # every rank its own batch
        sync.all_reduce()
        opt.step(clip_norm=0.05)
        norms.append(float(opt.last_grad_norm))
    q.put((rank, norms, opt.flat.detach().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_with_groups_and_a_clip_stay_bit_identical():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1] and all(n > 0.05 for n in res[0][1])      # the same norm on both ranks, clipping
    assert (res[0][2] == res[1][2]).all()
