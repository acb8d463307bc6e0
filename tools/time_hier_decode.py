#!/usr/bin/env python3
"""Greedy decode of the hierarchical decoder on one MI355X: HierMPNDecoder.decode with the synthetic graph batch
(ggpm_amd.synth_graph.SynthHierGraphBatch).  The sibling of tools/time_decode.py, with its shapes.

    python tools/time_hier_decode.py [--reps 5]

Shapes: LSTM H 250 (latent 24) and GRU H 300 (latent 32), diterT 1, diterG 3; a vocabulary of 500 motifs x 1500
attachments; B = 20 and 32; max_decode_step 100; beam 5.  Weights are seeded.  The graph batch is given room for 600 atoms
per molecule (IncGraph's default of 100 ends a decode of 100 steps with its IndexError).  One JSON line: per case the
median ms per batch over the repetitions after a warm-up, molecules/s, atoms and motifs per molecule, steps per batch,
launches / uploads / device-to-host copies per step, the host's share (time outside the blocking copies against time
blocked in them), and -- from one more, event-timed repetition -- the share of the device time spent in the atom step.
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
from hier_decode_fixtures import hier_decoder  # noqa: E402
from ggpm_amd import hier_decode as HD  # noqa: E402
from ggpm_amd.synth_graph import SynthHierGraphBatch  # noqa: E402

TOPO_BIAS = 0.0
DITER_G = 3
CASES = [("lstm_h250", "LSTM", 250, 24), ("gru_h300", "GRU", 300, 32)]


def roomy(*a, **k):
    return SynthHierGraphBatch(*a, max_nodes=600, max_edges=1800, **k)


def atom_share(d, z):
    """one decode with events around every device phase -> the atom step's share of the device time"""
    run = HD._Decode(d, roomy, z, 100, 5)
    run.be.spans = []
    with torch.no_grad():
        run.run()
    torch.cuda.synchronize()
    ms = {"atom": 0.0, "rest": 0.0}
    for name, a, b in run.be.spans:
        ms[name] += a.elapsed_time(b)
    return ms["atom"] / max(ms["atom"] + ms["rest"], 1e-9), ms["atom"] + ms["rest"]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    out = {"tool": "time_hier_decode", "topo_bias": TOPO_BIAS, "diterG": DITER_G, "max_decode_step": 100, "beam": 5,
           "reps": reps, "cases": {}}
    for name, rnn, H, L in CASES:
        d = hier_decoder(rnn, H, L, 500, 1500, 1, DITER_G, 3, TOPO_BIAS).to("cuda:0")
        for B in (20, 32):
            rs = np.random.RandomState(B)
            z = tuple(torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).cuda() for _ in range(3))
            d.decode(None, z, max_decode_step=100, graph_batch_factory=roomy)        # warm-up
            times, waits = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results, mols = d.decode(None, z, max_decode_step=100, graph_batch_factory=roomy)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                waits.append(sum(s["wait_s"] for s in d.last_decode_stats))
            st = d.last_decode_stats
            ms = 1e3 * statistics.median(times)
            wait = 1e3 * statistics.median(waits)
            motifs = np.mean([sum(1 for e in r if "Attaching Fragment" in e) for r in results])
            atoms = np.mean([len(m.split("|")[0]) for m in mols])
            share, dev_ms = atom_share(d, z)
            out["cases"]["%s_B%d" % (name, B)] = {
                "ms_per_batch": round(ms, 2), "molecules_per_s": round(B / ms * 1e3, 1), "steps": len(st),
                "mean_motifs_per_molecule": round(float(motifs), 2), "mean_atoms_per_molecule": round(float(atoms), 1),
                "launches_per_step": round(np.mean([s["launches"] for s in st]), 2),
                "max_launches_per_step": max(s["launches"] for s in st),
                "uploads_per_step": round(np.mean([s["h2d"] for s in st]), 2),
                "d2h_per_step": round(np.mean([s["d2h"] for s in st]), 2), "max_d2h_per_step": max(s["d2h"] for s in st),
                "host_ms": round(ms - wait, 2), "blocked_in_copies_ms": round(wait, 2),
                "device_ms_in_phases": round(dev_ms, 2), "atom_step_share_of_device_time": round(share, 3),
                "ms_spread": [round(1e3 * min(times), 2), round(1e3 * max(times), 2)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
