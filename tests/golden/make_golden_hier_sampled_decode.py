#!/usr/bin/env python3
"""Golden fixtures of the hierarchical decoder's SAMPLED decode, produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_hier_sampled_decode.py      (build container only; needs the reference checkout)

``make_golden_hier_decode.run_case`` with the two changes of ``make_golden_sampled_decode`` made from outside: the decoder
it builds forwards ``decode`` with ``greedy=False`` (ggpm/decoder.py:371-374, 409-416), and ``torch`` inside ``ggpm.decoder``
records every ``torch.bernoulli`` and ``torch.multinomial`` call.  The same acceptance of a seed; the reference's
hierarchical decode catches nothing, so a run in which anything raised is refused by ``run_case`` itself.  Fixtures are
DATA; no reference source text is stored.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_hier_decode as mh  # noqa: E402
import make_golden_sampled_decode as ms  # noqa: E402

import torch  # noqa: E402

OUT = os.path.join(HERE, "hier_decode_sampled")
CASES = [
    # name, rnn, H, latent, diterT, diterG, B, n_motif, max_decode_step, topo_bias, first seed
    ("gru_h16_g3", "GRU", 16, 8, 1, 3, 4, 12, 30, 0.3, 2100),
    ("lstm_h16_g3", "LSTM", 16, 8, 1, 3, 4, 12, 30, 0.3, 2200),
]


def main():
    mg.import_reference()
    import ggpm.decoder as D
    import ggpm.inc_graph as IG
    base_tree, base_dec = D.IncTree, D.HierMPNDecoder
    os.makedirs(OUT, exist_ok=True)
    D.HierMPNDecoder = ms.sampled(D, "HierMPNDecoder")
    for (name, rnn, H, L, dT, dG, B, n_motif, max_step, bias, seed0) in CASES:
        for seed in range(seed0, seed0 + 300):
            rec = D.torch = ms.RecordingTorch()
            out, info = mh.run_case(D, IG, base_tree, rnn, H, L, dT, dG, B, n_motif, max_step, bias, seed)
            if out is None or ms.accept(rec, json.loads(str(out["results"]))) is not None:
                continue
            break
        else:
            raise RuntimeError("no seed for %s" % name)
        out.update(ms.draws(rec))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-14s seed=%d margin=%.2e nodes=%d atoms=%d bernoulli=%d multinomial=%d %s -> %.1f KB" % (
            name, seed, float(out["margin"]), len(out["tree_fnode"]), len(out["atom_fnode"]), len(rec.bernoulli_calls),
            len(rec.multinomial_calls), sorted(k for k, v in info.items() if v), os.path.getsize(path) / 1024))
    D.torch, D.HierMPNDecoder = torch, base_dec


if __name__ == "__main__":
    main()
