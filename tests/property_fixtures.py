"""Loading of the property fixtures (tests/golden/make_golden_propopt.py) for the CPU and GPU tests."""
import glob
import os

import numpy as np

# a sub-directory of their own: tests/golden/*.npz is what golden_utils.case_names lists as encoder fixtures
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "property")


def names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, prefix + "_*.npz")))


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def head_shapes(half, hidden):
    hidden = [hidden] if isinstance(hidden, int) else list(hidden)
    widths = [half] + hidden + [1]
    out = {}
    for head in ("homo_linear", "lumo_linear"):
        for i in range(len(widths) - 1):
            out["%s.linear.%d.weight" % (head, 3 * i)] = (widths[i + 1], widths[i])
            out["%s.linear.%d.bias" % (head, 3 * i)] = (widths[i + 1],)
    return out


def propopt_state_dict(rnn, H, L, n_motif, n_attach, tie, hidden, scaling, seed):
    """Seeded parameters of a HierPropOptVAE: the vae_* layout, the two heads, LossWeigh's fp64 log-variances."""
    from ggpm_amd.params import vae_param_shapes, tied_state_dict, seeded_state_dict
    sd = seeded_state_dict(vae_param_shapes(rnn, H, L, n_motif, n_attach), seed)
    if tie:
        sd = tied_state_dict(sd)
    for k, v in seeded_state_dict(head_shapes(L // 2, hidden), seed + 11, bias_scale=0.3).items():
        sd["property_optim." + k] = v
    if scaling:
        rs = np.random.RandomState(seed + 13)
        for k in ("homo_log_var", "lumo_log_var", "recon_log_var"):
            sd["loss_weigh." + k] = (0.5 * rs.standard_normal(1)).astype(np.float64)
    return sd


def targets(seed, B):
    rs = np.random.RandomState(seed + 17)
    return (rs.standard_normal(B) * 0.7 - 0.5).astype(np.float32), (rs.standard_normal(B) * 0.7 + 0.5).astype(np.float32)


class PropOptGolden:
    """One propopt_* fixture: the reference HierPropOptVAE's forward + backward on a synthetic batch."""

    def __init__(self, name):
        self.name, self.z = name, load(name)
        (self.H, self.latent, self.depthT, self.depthG, self.diterT, self.diterG, self.B, self.n_motif, self.n_attach,
         self.seed, m0, m1, tie, scaling) = [int(v) for v in self.z["meta"]]
        self.motifs, self.tie, self.scaling = (m0, m1), bool(tie), bool(scaling)
        self.rnn = str(self.z["rnn"])
        lh = [int(v) for v in self.z["linear_hidden"]]
        self.linear_hidden = lh[0] if bool(self.z["linear_hidden_is_int"]) else lh

    def args(self, vocab):
        class A:
            pass
        a = A()
        a.vocab, a.rnn_type, a.embed_size, a.hidden_size = vocab, self.rnn, self.H, self.H
        a.atom_vocab = type("V", (), {"size": lambda s: 38})()
        a.depthT, a.depthG, a.diterT, a.diterG = self.depthT, self.depthG, self.diterT, self.diterG
        a.dropout, a.latent_size, a.tie_embedding = 0.0, self.latent, self.tie
        a.linear_hidden_size, a.property_optim_step = self.linear_hidden, 20
        if self.scaling:
            a.loss_scaling = True
        return a

    def state_dict(self):
        return propopt_state_dict(self.rnn, self.H, self.latent, self.n_motif, self.n_attach, self.tie,
                                  self.linear_hidden, self.scaling, self.seed)

    def specs(self):
        from ggpm_amd import synth
        return synth.random_batch(self.seed, self.B, motifs=self.motifs, n_motif_vocab=self.n_motif,
                                  n_attach_vocab=self.n_attach)

    def metrics(self):
        return dict(zip([str(k) for k in self.z["metric_names"]], [float(v) for v in self.z["metric_values"]]))
