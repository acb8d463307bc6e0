"""CPU: the tree-only models 'prop' / 'prop-opt' (PropertyVAE, PropOptVAE, MotifDecoder) -- registry, state_dict
contract, the decoder bookkeeping against the reference's, what is out of scope raising, the head kernel's exports."""
import numpy as np
import pytest
import torch

from motif_fixtures import MotifGolden, names

CASES = names()


def test_fixtures_present():
    assert len(CASES) >= 6
    assert any(MotifGolden(n).kind == "prop-opt" and MotifGolden(n).scaling for n in CASES)
    assert any(int(MotifGolden(n).z["ref_assm_batch"].size) == 0 for n in CASES)


def test_opvnet_registry():
    from ggpm_amd.opvnet import OPVNet
    from ggpm_amd.property_vae import HierPropertyVAE, HierPropOptVAE, PropertyVAE, PropOptVAE
    assert OPVNet.get_model('prop') is PropertyVAE and OPVNet.get_model('prop-opt') is PropOptVAE
    assert OPVNet.get_model('hier-prop') is HierPropertyVAE and OPVNet.get_model('hier-prop-opt') is HierPropOptVAE
    assert sorted(OPVNet.MODEL_DICT) == ['hier-prop', 'hier-prop-opt', 'prop', 'prop-opt']


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_are_the_references(name):
    g = MotifGolden(name)
    m = g.model()
    assert sorted(m.state_dict().keys()) == sorted(str(k) for k in g.z["sd_keys"])
    # aliases and ties share storage exactly where the reference's do
    sd = m.state_dict(keep_vars=True)
    for k, src in zip(g.z["sd_keys"], g.z["sd_src"]):
        assert sd[str(k)] is sd[str(src)], (k, src)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("native", [False, True])
def test_schedule_reproduces_reference_bookkeeping(name, native):
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.motif_decoder import AssmPlan
    g = MotifGolden(name)
    specs = g.specs()
    tensors = synth.tensorize(specs)
    for i, k in enumerate(("fnode", "fmess", "agraph", "bgraph", "cgraph")):
        assert np.array_equal(np.asarray(tensors[0][i]), g.z["tree_" + k]), k
    S = DecodeSchedule.from_specs(specs, tensors, native=native)
    ref = g.ref_steps()
    assert len(S.steps) == len(ref)
    for st, (sn, sm) in zip(S.steps, ref):
        assert st["subnode"] == sn and st["submess"] == sm
    tb, tl = S.topo()
    assert tb == g.z["ref_topo_batch"].tolist() and tl == g.z["ref_topo_label"].tolist()
    cb, cc, ci = S.cls()
    assert (cb, cc, ci) == tuple(g.z["ref_" + k].tolist() for k in ("cls_batch", "cls_clab", "cls_ilab"))
    assert S.assm_batch() == g.z["ref_assm_batch"].tolist()
    assert S.max_cls_size == int(g.z["ref_max_cls_size"])
    ap = AssmPlan(S)
    assert ap.meta[:, 0].tolist() == g.z["ref_assm_n"].tolist()
    assert ap.meta[:, 3].tolist() == g.z["ref_assm_batch"].tolist()


def test_out_of_scope_entry_points_raise():
    g = MotifGolden("propopt_gru_s63")
    m = g.model()
    with pytest.raises(NotImplementedError):
        m.reconstruct(None, None)
    with pytest.raises(NotImplementedError):
        m.optimize_recs(None, None)
    p = MotifGolden("prop_gru_s60").model()
    with pytest.raises(NotImplementedError):
        p.reconstruct(None, None)
    with pytest.raises(NotImplementedError):
        p.decoder(None, None, None, None, [None], avg_loss=True)


def test_embed_size_must_equal_hidden_size():
    from ggpm_amd.motif_decoder import MotifDecoder
    from ggpm_amd.vocab import IndexPairVocab
    with pytest.raises(ValueError):
        MotifDecoder(IndexPairVocab(5, 15), None, "GRU", 12, 16, 16, 1, 1, 0.0)


def test_prop_opt_always_ties_embeddings():
    g = MotifGolden("propopt_gru_s63")
    a = g.args()
    a.tie_embedding = False
    from ggpm_amd.property_vae import PropOptVAE
    m = PropOptVAE(a)
    assert m.encoder.E_c is m.decoder.hmpn.E_c and m.encoder.E_i is m.decoder.hmpn.E_i


def test_library_exports_the_head_kernel():
    from ggpm_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "ggpm_motif_assm_forward") and hasattr(lib, "ggpm_motif_assm_backward")
