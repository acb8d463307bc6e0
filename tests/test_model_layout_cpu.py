"""CPU: the parameter layout of the four VAE models is pinned -- ``named_parameters()`` (names and shapes) and the keys
of ``state_dict()``, in order, against tests/golden/model_layouts.json.  The order of ``parameters()`` is the layout of
FlatAdam's flat buffer and of the parameter tuple ``bound_loss`` hands to its first node, and the order in which the
sub-modules are constructed is the order in which they draw their initial weights from torch's generator, so a seeded run
depends on both.  (No digests of initial values: they would tie the test to one torch build.)

The fixture holds, per case, ``state_dict``: [key, shape] in order, and ``not_parameters``: the keys among them that
``named_parameters()`` does not list (the aliases ``rnn_cell`` / ``E_assm`` and the second name of a tied embedding); the
parameters are the other entries, in the same order."""
import json
import os

import pytest

from golden_utils import VaeGolden
from motif_fixtures import MotifGolden
from property_fixtures import PropOptGolden

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_layouts.json")


def _bag(kind):
    """The argument bag of the smallest golden case of ``kind`` (every one has hidden_size 16)."""
    from ggpm_amd.vocab import IndexPairVocab
    if kind == "hier-prop":
        g = VaeGolden("vae_gru_s40")
        return g.args(IndexPairVocab(g.n_motif, g.n_attach))
    if kind == "hier-prop-opt":
        g = PropOptGolden("propopt_gru_s50")
        return g.args(IndexPairVocab(g.n_motif, g.n_attach))
    return MotifGolden({"prop": "prop_gru_s60", "prop-opt": "propopt_gru_s63"}[kind]).args()


# the bag as the fixture has it (untied except prop-opt's, which says tied; latent 16 = hidden for the plain pair, 8 for the
# -opt pair; no LossWeigh), then one field changed: the embeddings tied or not (PropOptVAE ties them whatever the bag says),
# a latent width other than the hidden size (W_root exists), LossWeigh present
CASES = [("hier-prop", {}), ("hier-prop", dict(tie_embedding=True)), ("hier-prop", dict(latent_size=8)),
         ("hier-prop-opt", {}), ("hier-prop-opt", dict(tie_embedding=True)), ("hier-prop-opt", dict(loss_scaling=True)),
         ("prop", {}), ("prop", dict(tie_embedding=True)), ("prop", dict(latent_size=8)),
         ("prop-opt", {}), ("prop-opt", dict(tie_embedding=False)), ("prop-opt", dict(loss_scaling=True))]


def case_id(kind, changed):
    return kind + "".join("/%s=%s" % kv for kv in changed.items())


def layout(kind, changed):
    """(the [name, shape] list of ``named_parameters()``, the [key, shape] list of ``state_dict()``)"""
    from ggpm_amd.opvnet import OPVNet
    args = _bag(kind)
    for k, v in changed.items():
        setattr(args, k, v)
    model = OPVNet.get_model(kind)(args)
    return ([[k, list(p.shape)] for k, p in model.named_parameters()],
            [[k, list(v.shape)] for k, v in model.state_dict().items()])


@pytest.mark.parametrize("kind,changed", CASES, ids=[case_id(*c) for c in CASES])
def test_parameter_and_state_dict_order_are_the_recorded_ones(kind, changed):
    with open(FIXTURE) as f:
        want = json.load(f)[case_id(kind, changed)]
    parameters, state_dict = layout(kind, changed)
    assert state_dict == want["state_dict"]
    assert parameters == [e for e in want["state_dict"] if e[0] not in want["not_parameters"]]
