#!/usr/bin/env python3
"""Time the property features on the GPU (one JSON line per measurement, plus a summary):

  search:    the one-launch latent search (ggpm_property_latent_search) against a torch-on-GPU restatement of the
             reference's per-molecule loop (ggpm/property_control.py: one molecule at a time, a handful of small torch
             launches and host reads of the loss per step), latent 24, heads [64, 64], B = 20, ``soft`` and ``fixed``
             with 50 steps.  Reported per molecule-step for the loop, per step for the whole batch for the launch.
  fine-tune: the HierPropOptVAE training step (forward + backward) against the HierPropertyVAE step on the same
             fixture batch (tests/golden/vae_gru_s42: H 300, latent 32, 4 molecules).

    python tools/time_property_search.py [--reps N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Args:
    def __init__(self, mode, steps):
        self.optimize_type, self.property_optim_step, self.patience = mode, steps, 5
        self.patience_threshold, self.property_delta, self.latent_lr, self.max_steps = 0.1, 0.1, 1.0, 10000


def torch_heads(opt, dev):
    """The same two heads as plain torch modules on the GPU (the reference's form)."""
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
        return m.eval()
    return seq(opt.homo_linear), seq(opt.lumo_linear)


def loop_step(fh, fl, h, l, th, tl, lr, norm):
    """One step of the reference's form: forward both heads, MSE, backward to the latent, the signed update."""
    h = h.clone().detach().requires_grad_(True)
    l = l.clone().detach().requires_grad_(True)
    oh, ol = fh(h)[..., -1], fl(l)[..., -1]
    lh = torch.nn.functional.mse_loss(oh, th)
    ll = torch.nn.functional.mse_loss(ol, tl)
    total = lh + ll
    total.backward()
    sh = 1 - 2 * (oh < th).to(h.dtype)
    sl = 1 - 2 * (ol < tl).to(l.dtype)
    if h.dim() == 2:
        sh, sl = sh[:, None], sl[:, None]
    return total, (h - sh * lr * h.grad).detach(), (l - sl * lr * l.grad).detach()


def torch_soft(fh, fl, z, th, tl, half, lr=1.0, delta=0.1, patience=5, thr=0.1):
    steps = 0
    for r in range(z.shape[0]):
        h, l = z[r, :half], z[r, half:]
        prev, pat = 0.0, patience
        while pat > 0:
            total, hn, ln = loop_step(fh, fl, h, l, th[r], tl[r], lr, 2.0)
            steps += 1
            if total <= delta:                                    # host read, as the reference's loop
                break
            if total > prev or (abs(total - prev) / prev) <= thr:   # host reads
                pat -= 1
            else:
                pat = patience
            prev = total
            h, l = hn, ln
    return steps


def torch_fixed(fh, fl, z, th, tl, half, steps, lr=1.0):
    h, l = z[:, :half], z[:, half:]
    for _ in range(steps):
        _, h, l = loop_step(fh, fl, h, l, th, tl, lr, 2.0 / z.shape[0])
    return steps


def time_search(reps):
    from ggpm_amd.property import PropertyOptimizer
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = PropertyOptimizer(12, [64, 64], 0.1).to(dev).eval()
    holder = torch.nn.Module()
    holder.property_optim = opt
    fh, fl = torch_heads(opt, dev)
    B, half = 20, 12
    z = torch.randn(B, 24, device=dev)
    th, tl = torch.randn(B, device=dev) - 0.5, torch.randn(B, device=dev) + 0.5
    out = []
    for mode in ("soft", "fixed"):
        search = HierPropertyVAEOptimizer(holder, Args(mode, 50))
        fn = search._get_optimize_func()
        fn(z[:, :half], z[:, half:], th, tl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(z[:, :half], z[:, half:], th, tl)
        torch.cuda.synchronize()
        t_launch = (time.perf_counter() - t0) / reps
        launch_steps = int(search.steps_taken.max())           # the batch's longest trajectory
        run = (lambda: torch_soft(fh, fl, z, th, tl, half)) if mode == "soft" else \
            (lambda: torch_fixed(fh, fl, z, th, tl, half, 50))
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_steps = 0
        for _ in range(max(1, reps // 10)):
            n_steps = run()
        torch.cuda.synchronize()
        t_loop = (time.perf_counter() - t0) / max(1, reps // 10)
        mol_steps = n_steps if mode == "soft" else n_steps * B
        rec = {"what": "search", "mode": mode, "B": B, "latent": 24, "hidden": [64, 64],
               "launch_ms": t_launch * 1e3, "launch_us_per_step": t_launch * 1e6 / max(1, launch_steps),
               "launch_steps_max": launch_steps, "torch_loop_ms": t_loop * 1e3,
               "torch_loop_us_per_molecule_step": t_loop * 1e6 / max(1, mol_steps), "torch_loop_molecule_steps": mol_steps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def time_finetune(reps):
    from golden_utils import vae_model
    from ggpm_amd.property_vae import HierPropOptVAE
    from ggpm_amd.vocab import IndexPairVocab
    dev = torch.device("cuda:0")
    g, base, tensors, sch = vae_model("vae_gru_s42", dev)
    a = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    a.linear_hidden_size, a.property_optim_step = [64, 64], 50
    fine = HierPropOptVAE(a).to(dev)
    fine.load_state_dict(base.state_dict(), strict=False)
    homos, lumos = [0.1 * i for i in range(g.B)], [-0.1 * i for i in range(g.B)]

    def step_base():
        base.zero_grad()
        loss, _ = base(None, None, tensors, [None] * g.B, None, None, beta=g.beta, perturb_z=False, schedule=sch)
        loss.backward()

    def step_fine():
        fine.zero_grad()
        loss, _, _ = fine(None, None, tensors, [None] * g.B, homos, lumos, beta=g.beta, perturb_z=False, schedule=sch)
        loss.backward()

    times = {"base": [], "fine": []}
    for fn in (step_base, step_fine):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):                      # alternate the two, so that drift hits both alike
        for key, fn in (("base", step_base), ("fine", step_fine)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[key].append(time.perf_counter() - t0)
    rec = {"what": "finetune_step", "fixture": "vae_gru_s42", "reps": reps,
           "hierpropertyvae_ms_median": float(np.median(times["base"]) * 1e3),
           "hierpropoptvae_ms_median": float(np.median(times["fine"]) * 1e3)}
    rec["ratio"] = rec["hierpropoptvae_ms_median"] / rec["hierpropertyvae_ms_median"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_property_search.py needs the MI355X: there is no CPU timing")
    s = time_search(args.reps)
    f = time_finetune(args.reps)
    for r in s:
        print("search %-5s: one launch %.3f ms for the batch (%.2f us per step of all %d molecules); torch loop %.1f ms "
              "(%.0f us per molecule-step)" % (r["mode"], r["launch_ms"], r["launch_us_per_step"], r["B"],
                                                r["torch_loop_ms"], r["torch_loop_us_per_molecule_step"]))
    print("fine-tune step: HierPropOptVAE %.3f ms vs HierPropertyVAE %.3f ms (x%.3f)"
          % (f["hierpropoptvae_ms_median"], f["hierpropertyvae_ms_median"], f["ratio"]))


if __name__ == "__main__":
    main()
