#!/usr/bin/env python3
"""Golden fixtures of the tree-only decoder's SAMPLED decode, produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_sampled_decode.py      (build container only; needs the reference checkout)

Per case ``make_golden_decode.run_case`` runs as it does for the greedy fixtures -- seeded parameters and latents, the
synthetic graph batch, everything the reference's try/except covers watched -- with two changes made from outside: the
decoder it builds forwards ``decode`` with ``greedy=False`` (ggpm/decoder.py:984-987, 1024-1033), and the name
``torch`` inside ``ggpm.decoder`` is a stand-in that hands every attribute through to torch but records the input and
the output of each ``torch.bernoulli`` and ``torch.multinomial`` call.  The draws themselves are torch's, after
``torch.manual_seed(seed)``.

A seed is accepted only if at least one topology draw contradicts ``p > 0.5``, at least one drawn order is not the
identity, at least one molecule attaches another entry than the first of its top k, nothing was swallowed, and the
remaining decision margins (the gaps of every top-k selection, the gaps between distinct attachment scores) are at
least 1e-4 -- ``run_case`` checks the last two.  Recorded besides what the greedy fixtures hold: ``bernoulli`` and
``multinomial``, the calls in order as [input, output] (JSON).  Fixtures are DATA; no reference source text is stored.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_decode as md  # noqa: E402

import torch  # noqa: E402

OUT = os.path.join(HERE, "motif_decode_sampled")
CASES = [
    # name, rnn, H, latent, diterT, B, n_motif, max_decode_step, topo_bias, first seed
    ("gru_h16", "GRU", 16, 16, 1, 4, 12, 30, 0.3, 1100),
    ("lstm_h16_l8", "LSTM", 16, 8, 1, 4, 12, 30, 0.3, 1200),
]


class RecordingTorch:
    """``torch`` for the reference's decoder module: every attribute is torch's; bernoulli and multinomial are recorded"""

    def __init__(self):
        self.bernoulli_calls, self.multinomial_calls = [], []

    def __getattr__(self, name):
        return getattr(torch, name)

    def bernoulli(self, p, *a, **k):
        out = torch.bernoulli(p, *a, **k)
        self.bernoulli_calls.append([p.detach().double().tolist(), out.tolist()])
        return out

    def multinomial(self, w, n, replacement=False, **k):
        assert not replacement and n == w.shape[1]
        out = torch.multinomial(w, n, replacement=replacement, **k)
        self.multinomial_calls.append([w.detach().double().tolist(), out.tolist()])
        return out


def sampled(D, name):
    """a constructor of ``D.<name>`` whose instances forward ``decode`` as ``greedy=False``.  (The reference's constructors
    call ``super(<name>, self)`` through the module's global, so the class itself is in place while one is built.)"""
    base = getattr(D, name)

    def make(*a, **k):
        setattr(D, name, base)
        try:
            model = base(*a, **k)
        finally:
            setattr(D, name, make)
        real = model.decode
        model.decode = lambda mols, vecs, greedy=True, **kw: real(mols, vecs, greedy=False, **kw)
        return model
    return make


def accept(rec, results):
    """-> the reason a recorded run does not exercise the sampled path, or None"""
    if not any((p > 0.5) != (d > 0.5) for ps, ds in rec.bernoulli_calls for p, d in zip(ps, ds)):
        return "no topology draw against p > 0.5"
    if all(row == sorted(row) for _, rows in rec.multinomial_calls for row in rows):
        return "every drawn order is the identity"
    later = [e for r in results for e in r[1:] if "Attaching Fragment" in e
             and e["Attaching Fragment"][0] != e["top-5-inter-cands"][0][1]]
    if not later:
        return "no molecule attached another entry than the first"
    return None


def draws(rec):
    return {"bernoulli": np.array(json.dumps(rec.bernoulli_calls)),
            "multinomial": np.array(json.dumps(rec.multinomial_calls))}


def main():
    mg.import_reference()
    import ggpm.decoder as D
    base_tree, base_dec = D.IncTree, D.MotifDecoder
    os.makedirs(OUT, exist_ok=True)
    D.MotifDecoder = sampled(D, "MotifDecoder")
    for (name, rnn, H, L, dT, B, n_motif, max_step, bias, seed0) in CASES:
        for seed in range(seed0, seed0 + 300):
            rec = D.torch = RecordingTorch()
            out, info = md.run_case(D, base_tree, rnn, H, L, dT, B, n_motif, max_step, bias, seed)
            if out is None or accept(rec, json.loads(str(out["results"]))) is not None:
                continue
            break
        else:
            raise RuntimeError("no seed for %s" % name)
        out.update(draws(rec))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-12s seed=%d margin=%.2e nodes=%d bernoulli=%d multinomial=%d %s -> %.1f KB" % (
            name, seed, float(out["margin"]), len(out["tree_fnode"]), len(rec.bernoulli_calls),
            len(rec.multinomial_calls), sorted(k for k, v in info.items() if v), os.path.getsize(path) / 1024))
    D.torch, D.MotifDecoder = torch, base_dec


if __name__ == "__main__":
    main()
