"""No-grad versus grad-enabled forwards: ms per forward and peak allocated MiB, as one JSON line.

    python tools/time_inference.py [--reps N]

Rows: the configs[1] HierPropertyVAE forward (GRU and LSTM; eval mode, z = mean, diterT = 1 / diterG = 5 as the shipped
configurations), the configs[1] encoder (HierEncoderVAE) and the configs[4] encoder in fp32 and bf16 gate products.  Each
row times the same call with grad enabled (the training forward, its graph dropped afterwards) and under
torch.no_grad() (the forward-only forms); peak = torch.cuda.max_memory_allocated() above the allocation before the call.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ggpm_amd import synth  # noqa: E402
from ggpm_amd.decoder import DecodeSchedule  # noqa: E402
from ggpm_amd.property_vae import HierEncoderVAE, HierPropertyVAE, make_cuda  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {1: dict(hidden=300, depth=20, gen=(8, 12)), 4: dict(hidden=600, depth=30, gen=(46, 58))}


def _args(rnn, hidden, depth):
    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = rnn, hidden, hidden, depth, depth
    a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = 1, 5, 0.0, 32, False
    return a


def _measure(call, reps):
    """-> {"grad": {"ms", "peak_mib"}, "no_grad": {...}}: warm-up, then the peak of one call and the mean of `reps`."""
    out = {}
    for mode, ctx in (("grad", torch.enable_grad), ("no_grad", torch.no_grad)):
        with ctx():
            call()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with ctx():
            r = call()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del r
        t0 = time.perf_counter()
        for _ in range(reps):
            with ctx():
                r = call()
            del r
        torch.cuda.synchronize()
        out[mode] = {"ms": round((time.perf_counter() - t0) * 1e3 / reps, 3), "peak_mib": round(peak, 1)}
    out["ms_ratio"] = round(out["no_grad"]["ms"] / out["grad"]["ms"], 3)
    out["peak_ratio"] = round(out["no_grad"]["peak_mib"] / max(out["grad"]["peak_mib"], 1e-9), 3)
    return out


def vae_row(rnn, reps):
    c = CONFIGS[1]
    torch.manual_seed(0)
    model = HierPropertyVAE(_args(rnn, c["hidden"], c["depth"])).to(DEV).eval()
    specs = synth.random_batch(1000, 32, motifs=c["gen"], n_motif_vocab=500, n_attach_vocab=1500)
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    return _measure(lambda: model(None, None, tensors, [None] * 32, None, None, beta=0.1, perturb_z=False, schedule=sch),
                    reps)


def encoder_row(cfg, gate_dtype, reps):
    c = CONFIGS[cfg]
    torch.manual_seed(0)
    model = HierEncoderVAE(_args("GRU", c["hidden"], c["depth"])).to(DEV).eval()
    model.encoder.gate_dtype = gate_dtype
    tensors = make_cuda(synth.tensorize(synth.random_batch(1000, 32, motifs=c["gen"], n_motif_vocab=500,
                                                           n_attach_vocab=1500)))
    return _measure(lambda: model(tensors, perturb_z=False), reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = {"tool": "time_inference", "batch": 32, "reps": a.reps,
           "vae_configs1_gru": vae_row("GRU", a.reps), "vae_configs1_lstm": vae_row("LSTM", a.reps),
           "encoder_configs1_f32": encoder_row(1, "f32", a.reps),
           "encoder_configs4_f32": encoder_row(4, "f32", max(1, a.reps // 3)),
           "encoder_configs4_bf16": encoder_row(4, "bf16", max(1, a.reps // 3))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
