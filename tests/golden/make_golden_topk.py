#!/usr/bin/env python3
"""Golden fixtures of the two top-k selections of the greedy decode, produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_topk.py      (build container only; needs the reference checkout)

Per case the seeded score rows and the ragged owner table of ``tests/decode_kernel_oracle.topk_inputs`` go, as fp64
tensors, through
  * the reference's own ``nnutils.hier_topk`` with an ``IndexPairVocab`` built from that owner table, and
  * the root selection of the reference's ``MotifDecoder.decode`` (ggpm/decoder.py:914-933): a small reference decoder
    whose ``get_cls_score`` hands back the case's rows runs ``decode`` with ``max_decode_step=0``, and the root motif and
    the 'top-5-root-attachments' entries of its results are read back (so the root is recorded with k = 5, whatever the
    case's k; the graph batch is ``ggpm_amd.synth_graph.SynthGraphBatch``, as in make_golden_decode.py).
Recorded per case: meta (n_cls, n_icls, k, the root's k, M, seed, the cap of attachments per motif or 0), the owner array
and the two outputs as [M, 3k] fp64 (scores | motifs | attachments).  The inputs are regenerated from the seed.  Fixtures
are DATA; no reference source text is stored.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)

import torch  # noqa: E402

import decode_kernel_oracle as O  # noqa: E402
from ggpm_amd.synth_graph import SynthGraphBatch  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

OUT = O.TOPK_DIR
CASES = [c for c in O.TOPK_CASES if c[:3] in ((12, 36, 5), (300, 900, 5), (257, 513, 16), (40, 130, 16))]
M = 7
K_ROOT = 5


def reference_root(D, vocab, cls, icls):
    """(scores [M, 5], motifs [M, 5], attachments [M, 5]) as the reference's decode reports the root"""
    from ggpm.vocab import common_atom_vocab
    model = D.MotifDecoder(vocab, common_atom_vocab, "GRU", 8, 8, 8, 1, 1, 0.0)
    model.eval()
    model.get_cls_score = lambda src, bidx, vecs, labs: (torch.from_numpy(cls).double(), torch.from_numpy(icls).double())
    D.IncGraph = SynthGraphBatch
    D.Chem = types.SimpleNamespace(MolFromSmiles=lambda s: s)
    vecs = tuple(torch.zeros(len(cls), 8) for _ in range(3))
    with torch.no_grad():
        results, _ = model.decode(None, vecs, greedy=True, max_decode_step=0, beam=K_ROOT)
    S, C, A = np.zeros((len(cls), K_ROOT)), np.zeros((len(cls), K_ROOT)), np.zeros((len(cls), K_ROOT))
    for r, res in enumerate(results):
        C[r] = vocab[(res[0]["root"], "a0")][0]
        for q, (ismiles, score) in enumerate(res[0]["top-5-root-attachments"]):
            A[r, q], S[r, q] = vocab[("m0", ismiles)][1], float(score)
        assert res[0]["Attaching Fragment"]["attachment"] == res[0]["top-5-root-attachments"][0][0]
    return S, C, A


def main():
    mg.import_reference()
    import ggpm.decoder as D
    import ggpm.nnutils as NN
    os.makedirs(OUT, exist_ok=True)
    for n_cls, n_icls, k, cap, seed in CASES:
        cls, icls, owner = O.topk_inputs(n_cls, n_icls, k, seed, M, cap)
        vocab = IndexPairVocab(n_cls, n_icls, owner)
        with torch.no_grad():
            s, c, a = NN.hier_topk(torch.from_numpy(cls).double(), torch.from_numpy(icls).double(), vocab, k)
        hier = np.concatenate([s.numpy().astype(np.float64), np.asarray(c, np.float64), np.asarray(a, np.float64)], axis=1)
        root = np.concatenate(reference_root(D, vocab, cls, icls), axis=1)
        path = os.path.join(OUT, "c%d_i%d_k%d.npz" % (n_cls, n_icls, k))
        np.savez_compressed(path, meta=np.array([n_cls, n_icls, k, K_ROOT, M, seed, cap or 0], np.int64),
                            owner=owner.astype(np.int64), hier=hier, root=root)
        print("%-18s seed=%d -> %.1f KB" % (os.path.basename(path), seed, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
