"""Loading of the per-molecule likelihood fixtures (tests/golden/make_golden_mol_likelihood.py) for the CPU and GPU tests."""
import glob
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol_likelihood")
# model kinds (ggpm_amd.opvnet.OPVNet.get_model) a fixture's weights fit: the property heads of the -opt models play no part
# in log_likelihood and keep their initial values; PropOptVAE always ties its embeddings, so only a tied fixture fits it
KINDS = {"hier": ("hier-prop", "hier-prop-opt"), "motif": ("prop", "prop-opt")}


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def cases():
    """(fixture name, model kind) pairs: every fixture with every model class its weights fit"""
    out = []
    for n in names():
        g = LLGolden(n)
        out += [(n, kind) for kind in KINDS[g.decoder] if kind != "prop-opt" or g.tie]
    return out


class LLGolden:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        (self.H, self.latent, self.depthT, self.depthG, self.diterT, self.diterG, self.B, self.n_motif, self.n_attach,
         self.seed, self.bseed, m0, m1, tie, self.K) = [int(v) for v in self.z["meta"]]
        self.motifs, self.tie = (m0, m1), bool(tie)
        self.decoder, self.rnn = str(self.z["decoder"]), str(self.z["rnn"])

    def specs(self):
        from ggpm_amd import synth
        return synth.random_batch(self.bseed, self.B, motifs=self.motifs, n_motif_vocab=self.n_motif,
                                  n_attach_vocab=self.n_attach)

    def args(self, dropout=0.0):
        from ggpm_amd.vocab import IndexPairVocab

        class A:
            pass
        a = A()
        a.vocab, a.rnn_type, a.embed_size, a.hidden_size = IndexPairVocab(self.n_motif, self.n_attach), self.rnn, self.H, self.H
        a.atom_vocab = type("V", (), {"size": lambda s: 38})()
        a.depthT, a.depthG, a.diterT, a.diterG = self.depthT, self.depthG, self.diterT, self.diterG
        a.dropout, a.latent_size, a.tie_embedding = dropout, self.latent, self.tie
        a.linear_hidden_size, a.property_optim_step, a.loss_scaling = 8, 20, False
        return a

    def state_dict(self, model):
        from ggpm_amd.params import vae_param_shapes, tied_state_dict, seeded_state_dict
        if self.decoder == "hier":
            sd = seeded_state_dict(vae_param_shapes(self.rnn, self.H, self.latent, self.n_motif, self.n_attach), self.seed)
            return {k: torch.from_numpy(v) for k, v in (tied_state_dict(sd) if self.tie else sd).items()}
        shapes = dict((k, tuple(v.shape)) for k, v in model.state_dict().items())
        sd = seeded_state_dict(OrderedDict((str(k), shapes[str(k)]) for k in self.z["param_names"]), self.seed)
        return OrderedDict((str(k), torch.from_numpy(np.array(sd[str(s)]))) for k, s in zip(self.z["sd_keys"], self.z["sd_src"]))

    def model(self, kind, dropout=0.0):
        """The model class of ``kind`` with the fixture's encoder, latent-head and decoder weights, in eval mode."""
        from ggpm_amd.opvnet import OPVNet
        torch.manual_seed(self.seed)            # (the property heads' initial values)
        m = OPVNet.get_model(kind)(self.args(dropout))
        res = m.load_state_dict(self.state_dict(m), strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.", "property_optim.")) for k in res.missing_keys), \
            res.missing_keys
        return m.eval()

    def batch(self):
        """(the tuple ``model(*batch)`` takes, its DecodeSchedule) as ggpm_amd.synth builds the fixture's batch"""
        from ggpm_amd import synth
        from ggpm_amd.decoder import DecodeSchedule, synth_orders
        specs = self.specs()
        tensors = synth.tensorize(specs)
        orders = synth_orders(specs, tensors[0][-1]) if self.decoder == "motif" else [None] * self.B
        return (None, None, tensors, orders, [0.0] * self.B, [0.0] * self.B), DecodeSchedule.from_specs(specs, tensors)
