"""The sampled-decode fixtures (tests/golden/make_golden_sampled_decode.py and its hierarchical counterpart): loading, the
recorded draws as a replay sampler, and what the sampled-decode tests of both decoders share."""
import glob
import json
import os

import numpy as np

import decode_fixtures as DF
import hier_decode_fixtures as HF
import sample_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
DIRS = {"motif": os.path.join(HERE, "golden", "motif_decode_sampled"),
        "hier": os.path.join(HERE, "golden", "hier_decode_sampled")}
SEED = 0x5EEDC0DE12345678        # the stream seed of the tests that draw (64 bits: both halves are in use)


def cases():
    return [(kind, os.path.basename(p)[:-4]) for kind in ("motif", "hier")
            for p in sorted(glob.glob(os.path.join(DIRS[kind], "*.npz")))]


class _Draws:
    def _load_draws(self):
        self.bernoulli, self.multinomial = (json.loads(str(self.z[k])) for k in ("bernoulli", "multinomial"))

    def replay(self):
        return SO.Replay(self.bernoulli, self.multinomial, DF.TOL)


class MotifSampled(DF.DecodeGolden, _Draws):
    kind = "motif"

    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(DIRS["motif"], name + ".npz"))
        (self.H, self.L, self.diterT, self.B, self.n_motif, self.n_attach, self.max_step, self.beam,
         self.seed) = [int(v) for v in self.z["meta"]]
        self.rnn, self.topo_bias = str(self.z["rnn"]), float(self.z["topo_bias"])
        for k in ("results", "mols", "cands", "ops", "features"):
            setattr(self, k, json.loads(str(self.z[k])))
        self._load_draws()


class HierSampled(HF.HierDecodeGolden, _Draws):
    kind = "hier"

    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(DIRS["hier"], name + ".npz"))
        (self.H, self.L, self.diterT, self.diterG, self.B, self.n_motif, self.n_attach, self.max_step, self.beam,
         self.seed) = [int(v) for v in self.z["meta"]]
        self.rnn, self.topo_bias = str(self.z["rnn"]), float(self.z["topo_bias"])
        for k in ("results", "mols", "cands", "ops", "add_mol", "features"):
            setattr(self, k, json.loads(str(self.z[k])))
        self._load_draws()


def load(kind, name):
    return (MotifSampled if kind == "motif" else HierSampled)(name)


def module(kind):
    from ggpm_amd import hier_decode, motif_decode
    return motif_decode if kind == "motif" else hier_decode


def graph_batch(kind):
    from ggpm_amd.synth_graph import SynthGraphBatch, SynthHierGraphBatch
    return SynthGraphBatch if kind == "motif" else SynthHierGraphBatch


def oracle_backend(kind):
    import decode_kernel_oracle as O
    import hier_decode_kernel_oracle as HO
    return O.OracleBackend if kind == "motif" else HO.OracleBackend


def decode_sampled(g, dec, latents, rows=None, **kw):
    """``decode_sampled`` of ``g``'s decoder at the fixture's step limit and beam, on the molecules ``rows`` (default all)"""
    if rows is not None:
        latents = tuple(v[list(rows)] for v in latents)
    return module(g.kind).decode_sampled(dec, None, latents, max_decode_step=g.max_step, beam=g.beam,
                                         graph_batch_factory=graph_batch(g.kind), **kw)


def own(entries):
    """a molecule's results without what depends on its place in a batch: the atom ids of the shared graph batch (the
    first halves of an attachment's ``inter_label`` pairs, the root's atoms) and the empty steps after its last one"""
    out = []
    for e in DF.norm(entries):
        e = dict(e)
        a = e.get("Attaching Fragment")
        if isinstance(a, dict):
            e["Attaching Fragment"] = {k: v for k, v in a.items() if k != "attachment-points"}
            e["root atoms"] = len(a["attachment-points"][0]) if "attachment-points" in a else None
        elif a is not None:
            e["Attaching Fragment"] = [a[0], a[1], [p for _, p in a[2]], a[3]]
        out.append(e)
    while out and set(out[-1]) <= {"partial-graph"}:
        out.pop()
    return out
