"""Loading of the ``bound_loss`` fixtures (tests/golden/make_golden_mol_objective.py) for the CPU and GPU tests: one file per
likelihood case and objective variant; model and batch are the likelihood fixture's (mol_likelihood_fixtures.LLGolden)."""
import glob
import os

import numpy as np

import mol_likelihood_fixtures as LF

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol_objective")
VARIANTS = ("elbo_b03_w", "iwae", "iwae_w")


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


class ObjGolden:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.case, self.variant = name.split("__")
        self.objective, self.beta = str(self.z["objective"]), float(self.z["beta"])
        self.weights = self.z["weights"].tolist() if int(self.z["weighted"]) else None
        self.ll = LF.LLGolden(self.case)

    def grads(self, which):
        """{parameter name: the reference's gradient}, ``which`` = 32 or 64 (the precision of the run; stored as float32)"""
        pre = "grad%d/" % which
        return {k[len(pre):]: self.z[k] for k in self.z.files if k.startswith(pre)}


def cases():
    """(fixture name, model kind) pairs: every fixture with every model class its weights fit"""
    kinds = dict()
    for case, kind in LF.cases():
        kinds.setdefault(case, []).append(kind)
    return [(n, kind) for n in names() for kind in kinds[n.split("__")[0]]]
