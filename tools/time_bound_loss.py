"""``bound_loss`` + ``backward`` with K samples beside the training step ``model(*batch)`` + ``backward``: ms per step and peak
MiB, as one JSON line.

    python tools/time_bound_loss.py [--reps N] [--warmup N] [--objective iwae|elbo|tcvae] [--ks 1,4,16]

Rows: the configs[1] HierPropertyVAE (hidden 300, depth 20, diterT 1 / diterG 5, latent 32; B 32; GRU and LSTM; eval mode, no
dropout), K in {1, 4, 16}.  ``bound_ms`` is one ``model.bound_loss(batch, n_samples=K, objective="iwae", seed=...)`` followed
by ``loss.backward()`` -- one encoder pass and one atom-level pass each way, K passes of the tree-side levels and the heads;
``train_ms`` is ``model(*batch, beta=0.1)`` followed by ``backward()``, the step the K = 1 figure is to be read against.
Gradients are dropped (``zero_grad(set_to_none=True)``) before every step.  The two are timed in alternation, `reps` windows
each after `warmup` untimed rounds; a window is `calls` steps back to back between two device synchronisations, and the
figures are per step: the median over the windows, with the fastest and the slowest window beside it.  ``*_peak_mib`` is
``torch.cuda.max_memory_allocated`` over one step after a reset.  ``--objective elbo`` times the K-sample ELBO instead and
``--objective tcvae`` the beta-TCVAE loss (alpha 1, beta 4, gamma 1, dataset_size 250000), whose figure is to be read against
the ``elbo`` one of the same K; ``--ks`` replaces the list of K.  No threshold: the tool reports.
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
from ggpm_amd.property_vae import HierPropertyVAE  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

DEV = torch.device("cuda:0")
B, KS = 32, (1, 4, 16)


def _args(rnn):
    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = rnn, 300, 300, 20, 20
    a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = 1, 5, 0.0, 32, False
    return a


def _timed(call, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def _peak_mib(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    call()
    torch.cuda.synchronize()
    return round(torch.cuda.max_memory_allocated(DEV) / 2 ** 20, 1)


OBJECTIVES = {"iwae": dict(objective="iwae"), "elbo": dict(objective="elbo"),
              "tcvae": dict(objective="tcvae", beta=4.0, dataset_size=250000)}


def row(rnn, K, reps, warmup, calls, objective="iwae"):
    torch.manual_seed(0)
    model = HierPropertyVAE(_args(rnn)).to(DEV).eval()
    specs = synth.random_batch(1000, B, motifs=(8, 12), n_motif_vocab=500, n_attach_vocab=1500)
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    batch = (None, None, tensors, [None] * B, None, None)

    def bound():
        model.zero_grad(set_to_none=True)
        model.bound_loss(batch, n_samples=K, seed=7, schedule=sch, **OBJECTIVES[objective])[0].backward()

    def train():
        model.zero_grad(set_to_none=True)
        model(*batch, beta=0.1, perturb_z=True, schedule=sch)[0].backward()

    a, b = [], []
    for r in range(warmup + reps):
        ta, tb = _timed(bound, calls), _timed(train, calls)
        if r >= warmup:
            a.append(ta)
            b.append(tb)
    ba, tr = statistics.median(a), statistics.median(b)
    spread = lambda v: [round(min(v), 3), round(max(v), 3)]
    return {"K": K, "bound_ms": round(ba, 3), "bound_min_max": spread(a), "train_ms": round(tr, 3), "train_min_max": spread(b),
            "ratio": round(ba / tr, 3), "bound_peak_mib": _peak_mib(bound), "train_peak_mib": _peak_mib(train)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="steps per timed window (default: 8 for K = 1, 4 for K = 4, 2 for K = 16)")
    ap.add_argument("--objective", choices=sorted(OBJECTIVES), default="iwae", help="what bound_loss computes (default: iwae)")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="comma-separated n_samples (default: %(default)s)")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    res = {"tool": "time_bound_loss", "objective": a.objective, "batch": B, "reps": a.reps, "warmup": a.warmup,
           "calls": a.calls or "8/4/2"}
    for rnn in ("GRU", "LSTM"):
        res["configs1_" + rnn.lower()] = [row(rnn, K, a.reps, a.warmup, a.calls or (8 if K < 4 else 4 if K < 16 else 2), a.objective)
                                          for K in ks]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
