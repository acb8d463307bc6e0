"""The step tail behind backward -- clip_grad_norm_ + Adam -- on the configs[1] HierPropertyVAE parameter set with random
gradients (no forward pass): median host-issue ms and median device ms (HIP events) per leg, one JSON line per leg.

    python tools/time_optimizer.py [--reps N] [--warmup W]

Legs: (a) torch's clip_grad_norm_(model.parameters(), 20.0) + torch.optim.Adam(model.parameters(), fused=True).step();
(b) FlatAdam.step(clip_norm=20.0); (c) FlatAdam.step(), the launch bench.py times; (d) (b) with four parameter groups (the
split of vae_fine_tune_indv_opt.py by name: 'decoder', the rest, and -- this model has no property heads -- 'R_mean' and 'R_var'
in their place); (e) (b) with the non-finite guard; (f) (e) with the EMA of the parameters in the same launch.  Last line: FlatAdam.param_norm() + grad_norm() against the scripts' per-parameter .item() loops, both read
on the host.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ggpm_amd.optim import FlatAdam  # noqa: E402
from ggpm_amd.parallel import FlatGradSync  # noqa: E402
from ggpm_amd.property_vae import HierPropertyVAE  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

DEV = torch.device("cuda:0")
CLIP = 20.0


def _model():
    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = "GRU", 300, 300, 20, 20
    a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = 1, 5, 0.0, 32, False
    torch.manual_seed(0)
    return HierPropertyVAE(a).to(DEV)


def _flat(groups: bool, **features):
    model = _model()
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    pg = None
    if groups:
        named = list(model.named_parameters())
        keys = ("decoder", "R_mean", "R_var")
        pg = [{"params": [p for k, p in named if not any(key in k for key in keys)], "lr": 1e-3}]
        pg += [{"params": [p for k, p in named if key in k], "lr": lr} for key, lr in zip(keys, (5e-4, 2e-3, 3e-3))]
    opt = FlatAdam(sync, lr=1e-3, param_groups=pg, **features)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for v in sync.views:                                 # random gradients; the padding between parameters stays zero
        v.normal_(generator=gen)
    sync.pack()
    return model, sync, opt


def _time(call, reps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    host, ev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    dev = [a.elapsed_time(b) for a, b in ev]
    return {"host_issue_ms": round(statistics.median(host), 4), "device_ms": round(statistics.median(dev), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.reps < 50:
        ap.error("--reps: at least 50")
    base = {"tool": "time_optimizer", "reps": a.reps, "warmup": a.warmup, "clip_norm": CLIP}

    model = _model()
    params = list(model.parameters())
    gen = torch.Generator(device=DEV).manual_seed(1)
    grads = [torch.randn(p.shape, device=DEV, generator=gen) for p in params]
    topt = torch.optim.Adam(params, lr=1e-3, fused=True)

    def leg_a():
        for p, g in zip(params, grads):                  # (clip_grad_norm_ scales in place: the same gradient every time)
            p.grad = g
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        topt.step()
    base["parameters"], base["floats"] = len(params), sum(p.numel() for p in params)
    print(json.dumps(dict(base, leg="a: clip_grad_norm_ + torch.optim.Adam(fused=True)", **_time(leg_a, a.reps, a.warmup))))

    _, sync, opt = _flat(groups=False)
    base["flat_floats"] = sync.flat.numel()
    print(json.dumps(dict(base, leg="b: FlatAdam.step(clip_norm)", **_time(lambda: opt.step(clip_norm=CLIP), a.reps, a.warmup))))
    print(json.dumps(dict(base, leg="c: FlatAdam.step()", **_time(opt.step, a.reps, a.warmup))))
    # the guarded step and the guarded, averaging step: each still the partials launch and ONE update launch
    _, _, opt_g = _flat(groups=False, skip_nonfinite=True)
    print(json.dumps(dict(base, leg="e: FlatAdam(skip_nonfinite).step(clip_norm)",
                          **_time(lambda: opt_g.step(clip_norm=CLIP), a.reps, a.warmup))))
    _, _, opt_e = _flat(groups=False, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    print(json.dumps(dict(base, leg="f: FlatAdam(skip_nonfinite, ema_decay).step(clip_norm)",
                          **_time(lambda: opt_e.step(clip_norm=CLIP), a.reps, a.warmup))))
    assert opt_g.skipped_steps == 0 and opt_e.skipped_steps == 0
    _, sync4, opt4 = _flat(groups=True)
    print(json.dumps(dict(base, leg="d: FlatAdam.step(clip_norm), four groups",
                          **_time(lambda: opt4.step(clip_norm=CLIP), a.reps, a.warmup))))

    # the two norms the scripts print, read on the host both ways (wall ms, the reads included)
    def loops():
        return (math.sqrt(sum(p.norm().item() ** 2 for p in params)),
                math.sqrt(sum(p.grad.norm().item() ** 2 for p in params if p.grad is not None)))

    def flat_norms():
        pn, gn = opt.param_norm(), opt.grad_norm()
        return pn.item(), gn.item()
    rows = {}
    for name, call in (("item_loops_ms", loops), ("flat_norms_ms", flat_norms)):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        rows[name] = round(statistics.median(ts), 4)
    print(json.dumps(dict(base, leg="param_norm + grad_norm, read on the host", **rows)))


if __name__ == "__main__":
    main()
