#!/usr/bin/env python3
"""Greedy decode on one MI355X: MotifDecoder.decode with the synthetic graph batch (ggpm_amd.synth_graph).

    python tools/time_decode.py [--reps 5]

Shapes: the shipped tree-only config (LSTM, H 250, latent 24, diterT 1) and H 300 GRU (latent 32); a vocabulary of 500
motifs x 1500 attachments; B = 20 and 32; max_decode_step 100; beam 5.  Weights are seeded, the topology head's output
bias raised by TOPO_BIAS so that trees grow (the mean motifs per molecule is printed).  One JSON line: per case the median
ms per batch over the repetitions after a warm-up, molecules/s, steps per batch, launches / uploads / device-to-host
copies per step, and the host's share: time outside the blocking copies (bookkeeping, the graph batch, launch issue)
against time blocked in them (device work the host waits for, and the copies).
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from decode_fixtures import AtomVocab, state_dict  # noqa: E402
from ggpm_amd.motif_decoder import MotifDecoder  # noqa: E402
from ggpm_amd.synth_graph import SynthGraphBatch  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

TOPO_BIAS = 0.0
CASES = [("lstm_h250", "LSTM", 250, 24), ("gru_h300", "GRU", 300, 32)]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    out = {"tool": "time_decode", "topo_bias": TOPO_BIAS, "max_decode_step": 100, "beam": 5, "reps": reps, "cases": {}}
    for name, rnn, H, L in CASES:
        d = MotifDecoder(IndexPairVocab(500, 1500), AtomVocab(), rnn, H, H, L, 1, 1, 0.0)
        d.load_state_dict(state_dict(d, [k for k, _ in d.named_parameters()], 3, TOPO_BIAS), strict=True)
        d = d.eval().to("cuda:0")
        for B in (20, 32):
            rs = np.random.RandomState(B)
            z = tuple(torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).cuda() for _ in range(3))
            d.decode(None, z, max_decode_step=100, graph_batch_factory=SynthGraphBatch)        # warm-up
            times, waits = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results, _ = d.decode(None, z, max_decode_step=100, graph_batch_factory=SynthGraphBatch)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                waits.append(sum(s["wait_s"] for s in d.last_decode_stats))
            st = d.last_decode_stats
            ms = 1e3 * statistics.median(times)
            wait = 1e3 * statistics.median(waits)
            motifs = np.mean([sum(1 for e in r if "Attaching Fragment" in e) for r in results])
            out["cases"]["%s_B%d" % (name, B)] = {
                "ms_per_batch": round(ms, 2), "molecules_per_s": round(B / ms * 1e3, 1), "steps": len(st),
                "mean_motifs_per_molecule": round(float(motifs), 2),
                "launches_per_step": round(np.mean([s["launches"] for s in st]), 2),
                "max_launches_per_step": max(s["launches"] for s in st),
                "uploads_per_step": round(np.mean([s["h2d"] for s in st]), 2),
                "d2h_per_step": round(np.mean([s["d2h"] for s in st]), 2), "max_d2h_per_step": max(s["d2h"] for s in st),
                "host_ms": round(ms - wait, 2), "blocked_in_copies_ms": round(wait, 2),
                "ms_spread": [round(1e3 * min(times), 2), round(1e3 * max(times), 2)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
