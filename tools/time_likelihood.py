"""``log_likelihood`` with K samples versus K no-grad forwards of the same model: ms per call, as one JSON line.

    python tools/time_likelihood.py [--reps N] [--warmup N]

Rows: the configs[1] HierPropertyVAE (hidden 300, depth 20, diterT 1 / diterG 5, latent 32; B 32; GRU and LSTM; eval mode),
K in {1, 4, 16}.  ``likelihood_ms`` is one ``model.log_likelihood(batch, n_samples=K, seed=...)`` -- one encoder pass, one
atom-level pass, K passes of the tree-side levels and the heads; ``forwards_ms`` is K repetitions of the no-grad
``model(*batch, perturb_z=True)``, which is what a caller without the method would run (and which gives no per-molecule
figures).  The two are timed in alternation, `reps` windows each after `warmup` untimed rounds; a window is `calls`
calls back to back between two device synchronisations (so that it holds tens of milliseconds of work, not one call's), and
the figures are per call: the median over the windows, with the fastest and the slowest window beside it.
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


def row(rnn, K, reps, warmup, calls):
    torch.manual_seed(0)
    model = HierPropertyVAE(_args(rnn)).to(DEV).eval()
    specs = synth.random_batch(1000, B, motifs=(8, 12), n_motif_vocab=500, n_attach_vocab=1500)
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    batch = (None, None, tensors, [None] * B, None, None)

    def likelihood():
        return model.log_likelihood(batch, n_samples=K, seed=7, schedule=sch)

    def forwards():
        with torch.no_grad():
            for _ in range(K):
                model(*batch, beta=0.1, perturb_z=True, schedule=sch)

    stats = likelihood().stats
    a, b = [], []
    for r in range(warmup + reps):
        ta, tb = _timed(likelihood, calls), _timed(forwards, calls)
        if r >= warmup:
            a.append(ta)
            b.append(tb)
    la, fb = statistics.median(a), statistics.median(b)
    spread = lambda v: [round(min(v), 3), round(max(v), 3)]
    return {"K": K, "likelihood_ms": round(la, 3), "likelihood_min_max": spread(a), "forwards_ms": round(fb, 3),
            "forwards_min_max": spread(b), "ratio": round(la / fb, 3), "stats": stats}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (default: 8 for K = 1, 4 for K = 4, 2 for K = 16)")
    a = ap.parse_args()
    res = {"tool": "time_likelihood", "batch": B, "reps": a.reps, "warmup": a.warmup, "calls": a.calls or "8/4/2"}
    for rnn in ("GRU", "LSTM"):
        res["configs1_" + rnn.lower()] = [row(rnn, K, a.reps, a.warmup, a.calls or {1: 8, 4: 4, 16: 2}[K]) for K in KS]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
