"""CPU: the tree-only models' oracle (tests/motif_oracle.py) reproduces the reference's own steps (tests/golden/motif_vae):
loss, metrics and every gradient."""
import numpy as np
import pytest
import torch

import motif_oracle as mo
from motif_fixtures import MotifGolden, names


@pytest.mark.parametrize("name", names())
def test_oracle_matches_reference_fixture(name):
    g = MotifGolden(name)
    loss, metrics, grads = mo.run(g, torch.float64)
    g.check_step_values(float(loss), metrics, {k: (None if v is None else v.numpy()) for k, v in grads.items()})


def test_oracle_drop_hook_reaches_every_site():
    g = MotifGolden("prop_gru_s60")
    seen = set()

    def drop(site, x, step):
        seen.add(site)
        return x
    mo.run(g, torch.float64, drop=drop)
    assert seen == {"encoder.E_c", "encoder.E_i", "decoder.E_c", "decoder.W_o", "decoder.E_assm", "topoNN.2", "clsNN.2",
                    "iclsNN.2"}
