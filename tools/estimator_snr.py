"""Signal-to-noise ratio of the latent heads' gradient under the three estimators of ``bound_loss(objective="iwae")``, as one
JSON line.

    timeout -k 10 300 python tools/estimator_snr.py [--seeds R] [--warmup N]

Rows: the configs[1] HierPropertyVAE (hidden 300, depth 20, diterT 1 / diterG 5, latent 32; B 32; GRU; eval mode, no dropout;
the seeded initial weights of ``tools/time_bound_loss.py``), estimator in {reparam, stl, dreg} x K in {1, 4, 16}.  A row runs
``model.bound_loss(batch, n_samples=K, objective="iwae", seed=r, estimator=...)`` + ``backward`` for the seeds r = 0 .. R - 1
on one batch and reports
  snr_R_mean, snr_R_var  over the elements of the gradient of ``R_mean.weight`` / ``R_var.weight``: the mean of
                         |mean over seeds| / std over seeds (std with divisor R - 1; an element whose std is 0 is left out)
  ms                     the median over the seeds of one step, a host clock around the step ending in a device synchronise
  ess_mean               the mean over seeds and molecules of the effective sample size (``info.ess``; the importance weights
                         do not depend on the estimator, and the ``reparam`` call does not report them: null there)
One process, nothing is read from outside the repository.  No threshold: the tool reports (figures: DESIGN §24).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ggpm_amd import synth  # noqa: E402
from ggpm_amd.decoder import DecodeSchedule  # noqa: E402
from ggpm_amd.property_vae import ESTIMATORS, HierPropertyVAE  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

DEV = torch.device("cuda:0")
B, KS = 32, (1, 4, 16)
HEADS = ("R_mean", "R_var")


def _args(rnn):
    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = rnn, 300, 300, 20, 20
    a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = 1, 5, 0.0, 32, False
    return a


def snr(grads):
    """grads [R, ...] -> the mean over elements of |mean over seeds| / std over seeds, in fp64"""
    g = grads.double()
    mean, std = g.mean(dim=0).abs(), g.std(dim=0, unbiased=True)
    ok = std > 0
    return float((mean[ok] / std[ok]).mean()) if bool(ok.any()) else None


def row(model, batch, sch, estimator, K, seeds, warmup):
    def step(seed):
        model.zero_grad(set_to_none=True)
        loss, info = model.bound_loss(batch, n_samples=K, objective="iwae", seed=seed, schedule=sch, estimator=estimator)
        loss.backward()
        return info

    for r in range(warmup):
        step(1000 + r)
    grads, ms, ess = {h: [] for h in HEADS}, [], []
    for r in range(seeds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = step(r)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        for h in HEADS:
            grads[h].append(getattr(model, h).weight.grad.clone())
        if estimator != "reparam":
            ess.append(info.ess.double().mean())
    out = {"estimator": estimator, "K": K, "ms": round(statistics.median(ms), 3),
           "ess_mean": round(float(torch.stack(ess).mean()), 4) if ess else None}
    for h in HEADS:
        v = snr(torch.stack(grads[h]))
        out["snr_" + h] = None if v is None else round(v, 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.seeds < 2:
        ap.error("--seeds: a standard deviation needs at least 2")
    torch.manual_seed(0)
    model = HierPropertyVAE(_args("GRU")).to(DEV).eval()
    specs = synth.random_batch(1000, B, motifs=(8, 12), n_motif_vocab=500, n_attach_vocab=1500)
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    batch = (None, None, tensors, [None] * B, None, None)
    res = {"tool": "estimator_snr", "batch": B, "seeds": a.seeds, "warmup": a.warmup, "cell": "GRU",
           "rows": [row(model, batch, sch, e, K, a.seeds, a.warmup) for K in KS for e in ESTIMATORS]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
