#!/usr/bin/env python3
"""Time the guided latent search on the GPU (one JSON line):

  the one-launch search (ggpm_latent_search_guided, then ggpm_latent_search_select) against a torch-autograd loop over the
  same objective written here -- all K B rows batched, one backward and a handful of elementwise launches per step; not a
  product path --, for B = 32, K in {1, 8}, steps = 50, latent 24, heads [64, 64], with the standard-normal prior and with a
  64-component MixturePrior.  Both sides are timed from issue to a final synchronise, median over ``--reps`` runs.

    python tools/time_latent_search.py [--reps N]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HALF, HIDDEN, STEPS, LR, MOM, AW, PW = 32, 12, [64, 64], 50, 0.02, 0.9, 0.3, 0.1


def torch_heads(opt, dev):
    def seq(head):
        lins = head.linears()
        layers = []
        for lin in lins[:-1]:
            layers += [torch.nn.Linear(lin.in_features, lin.out_features), torch.nn.ReLU()]
        layers.append(torch.nn.Linear(lins[-1].in_features, 1))
        m = torch.nn.Sequential(*layers).to(dev)
        with torch.no_grad():
            for dst, src in zip([l for l in m if isinstance(l, torch.nn.Linear)], lins):
                dst.weight.copy_(src.weight)
                dst.bias.copy_(src.bias)
        return m.eval().requires_grad_(False)
    return seq(opt.homo_linear), seq(opt.lumo_linear)


def torch_loop(fh, fl, z0, mu, lv, th, tl, prior, K):
    """the same trajectory with autograd: J summed over the rows (the rows are independent), heavy-ball momentum"""
    v = z0.reshape(K * B, -1).clone()
    m = torch.zeros_like(v)
    mu, iv, th, tl = mu.repeat(K, 1), torch.exp(-lv).repeat(K, 1), th.repeat(K), tl.repeat(K)

    def objective(v):
        prop = (fh(v[:, :HALF])[:, 0] - th) ** 2 + (fl(v[:, HALF:])[:, 0] - tl) ** 2
        anchor = 0.5 * ((v - mu) ** 2 * iv).sum(1)
        if prior is None:
            pr = 0.5 * (math.log(2 * math.pi) + v * v).sum(1)
        else:
            a, mm, s = prior
            d = v[:, None, :] - mm[None]
            comp = torch.log_softmax(a, 0)[None] - 0.5 * (math.log(2 * math.pi) + s[None] + d * d * torch.exp(-s)[None]).sum(2)
            pr = -torch.logsumexp(comp, 1)
        return prop + AW * anchor + PW * pr

    for _ in range(STEPS):
        v = v.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(objective(v).sum(), v)
        m = MOM * m + g
        v = v.detach() - LR * m
    with torch.no_grad():
        J = objective(v).reshape(K, B)
        return v.reshape(K, B, -1)[J.argmin(0), torch.arange(B, device=v.device)]


def launches(opt, z0, mu, lv, th, tl, prior, K):
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    dev, L = z0.device, 2 * HALF
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    z_all, pred_all, terms_all = torch.empty(K, B, L, **f32), torch.empty(2, K * B, **f32), torch.empty(K, B, 3, **f32)
    J, n = torch.empty(K, B, **f32), torch.empty(K, B, **i32)
    best, latent, pred, terms = torch.empty(B, **i32), torch.empty(B, L, **f32), torch.empty(2, B, **f32), torch.empty(B, 3, **f32)
    heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
    mix = prior or (None, None, None)
    lib = _lib.load()
    _lib.check(lib.ggpm_latent_search_guided(
        K, B, F_._p(z0), L, HALF, F_._p(mu), F_._p(lv), ctypes.byref(heads[0]), ctypes.byref(heads[1]), F_._p(th), F_._p(tl),
        F_._p(mix[0]), F_._p(mix[1]), F_._p(mix[2]), 0 if prior is None else prior[0].numel(), LR, MOM, STEPS, -1.0, 1.0, 1.0,
        AW, PW, F_._p(z_all), F_._p(pred_all), F_._p(terms_all), F_._p(J), F_._p(n), F_._stream()), "latent_search_guided")
    _lib.check(lib.ggpm_latent_search_select(F_._p(J), F_._p(z_all), F_._p(pred_all), F_._p(terms_all), K, B, L, F_._p(best),
                                             F_._p(latent), F_._p(pred), F_._p(terms), F_._stream()), "latent_search_select")
    return latent


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_latent_search.py needs the MI355X: there is no CPU timing")
    from ggpm_amd.property import PropertyOptimizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = PropertyOptimizer(HALF, HIDDEN, 0.1).to(dev).eval()
    fh, fl = torch_heads(opt, dev)
    L = 2 * HALF
    mu, lv = 0.8 * torch.randn(B, L, device=dev), -torch.randn(B, L, device=dev).abs()
    th, tl = torch.randn(B, device=dev), torch.randn(B, device=dev)
    mixture = (torch.randn(64, device=dev), 0.7 * torch.randn(64, L, device=dev), 0.3 * torch.randn(64, L, device=dev))
    rows = []
    for K in (1, 8):
        z0 = (mu[None] + torch.exp(0.5 * lv)[None] * torch.randn(K, B, L, device=dev)).contiguous()
        z0[0] = mu
        for name, prior in (("standard_normal", None), ("mixture_64", mixture)):
            a = launches(opt, z0, mu, lv, th, tl, prior, K)
            b = torch_loop(fh, fl, z0, mu, lv, th, tl, prior, K)
            rows.append({"K": K, "prior": name,
                         "one_launch_ms": median_ms(lambda: launches(opt, z0, mu, lv, th, tl, prior, K), args.reps),
                         "torch_autograd_loop_ms": median_ms(lambda: torch_loop(fh, fl, z0, mu, lv, th, tl, prior, K),
                                                             max(1, args.reps // 4)),
                         "max_abs_difference_of_the_selected_latents": float((a - b).abs().max())})
    print(json.dumps({"what": "guided_latent_search", "B": B, "latent": L, "hidden": HIDDEN, "steps": STEPS, "reps": args.reps,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
