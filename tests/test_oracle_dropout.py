"""CPU: the oracle's dropout hook (``drop`` of oracle/ref_decoder.py and ref_encoder.py) -- inactive it changes nothing, it
is called at the reference's sites with the rows the schedule says, and the row layout the GPU tests assume for the
atom level's own masks matches the oracle's per-step order."""
import numpy as np
import pytest
import torch

from golden_utils import VaeGolden, vae_case_names
from ggpm_amd import synth
from oracle import ref_encoder as ref, ref_decoder as refd


def _vae_case(name):
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name)
    specs = g.specs()
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    tt, gt = ref.to_long_tensors(tensors[0]), ref.to_long_tensors(tensors[1])
    return g, tensors, sch, tt, gt, IndexPairVocab(g.n_motif, g.n_attach).mask


def _oracle_step(g, sch, tt, gt, mask, **kw):
    p = {k: torch.from_numpy(v).requires_grad_(True) for k, v in g.state_dict().items()}
    if g.tie:
        for k in ("E_c.0.weight", "E_i.0.weight"):
            p["encoder." + k] = p["decoder.hmpn." + k]
    loss, kl, accs, recon = refd.vae_forward(p, g.rnn, g.depthT, g.depthG, g.diterT, g.diterG, tt, gt, sch, mask, g.beta,
                                             **kw)
    loss.backward()
    return loss.detach(), kl.detach(), [float(a) for a in accs], p


@pytest.mark.parametrize("name", vae_case_names())
def test_identity_drop_leaves_the_oracle_bit_identical(name):
    g, _, sch, tt, gt, mask = _vae_case(name)
    seen = set()

    def identity(site, x, step):
        seen.add(site)
        return x

    a = _oracle_step(g, sch, tt, gt, mask)
    b = _oracle_step(g, sch, tt, gt, mask, drop=identity)
    assert seen == {"graph_encoder.W_o", "inter_encoder.W_o", "tree_encoder.W_o", "E_i", "W_i", "E_c", "W_c", "E_assm",
                    "topoNN.2", "clsNN.2", "iclsNN.2"}
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    for k, v in a[3].items():
        w = b[3][k]
        assert (v.grad is None) == (w.grad is None), k
        assert v.grad is None or torch.equal(v.grad, w.grad), k


@pytest.mark.parametrize("name", ["vae_gru_s40", "vae_lstm_s41"])
def test_drop_sites_see_the_rows_of_the_schedule(name):
    """Every call of ``drop``: its site, its step and its rows, summed per site against the schedule's counts -- the atom
    level's W_o over the atoms of each step (aoff[-1] in all), the tree-side embeddings and read-outs over every visit
    (n_inst), E_assm over every candidate atom, the heads over their prediction rows."""
    g, _, sch, tt, gt, mask = _vae_case(name)
    rows, per_step = {}, {}

    def count(site, x, step):
        rows[site] = rows.get(site, 0) + x.shape[0]
        per_step[(site, step)] = per_step.get((site, step), 0) + x.shape[0]
        return x

    _oracle_step(g, sch, tt, gt, mask, drop=count)
    aoff, n_inst = sch.plan["atom_off"], sch.plan["n_inst"]
    assert rows["graph_encoder.W_o"] == aoff[-1] == sum(len(st["atoms"]) for st in sch.steps)
    for t in range(len(sch.steps)):
        assert per_step.get(("graph_encoder.W_o", t), 0) == aoff[t + 1] - aoff[t], t
    for site in ("E_i", "W_i", "inter_encoder.W_o", "E_c", "W_c", "tree_encoder.W_o"):
        assert rows[site] == n_inst == sum(len(st["subnode"]) for st in sch.steps), site
    n_cand_atoms = sum(np.asarray(c).size for st in sch.steps for c, _, _, _ in st["assm"])
    assert rows["E_assm"] == n_cand_atoms
    tb, _ = sch.topo()
    cb, _, _ = sch.cls()
    assert rows["topoNN.2"] == len(tb)
    assert rows["clsNN.2"] == rows["iclsNN.2"] == len(cb)
    assert {s for s, t in per_step if t is None} == {"topoNN.2", "clsNN.2", "iclsNN.2"}


@pytest.mark.parametrize("name", vae_case_names())
def test_compact_row_base_maps_to_the_oracle_atom_order(name):
    """The atom level's compact form masks row aoff[t] + j of one [aoff[-1], H] call; the GPU tests take that row to be
    atom st["atoms"][j] of step t, the j-th row of the oracle's W_o call at step t.  The atom plan's offsets and the
    read-out's row -> atom table (plan["atoms_all"], what the node rows are gathered by) must say the same."""
    from ggpm_amd.atom_decode import AtomPlan
    g, tensors, sch, _, _, _ = _vae_case(name)
    n_gnodes, n_gmess = tensors[1][0].shape[0], tensors[1][1].shape[0]
    for full in (False, True):
        ap = AtomPlan(sch, n_gnodes, n_gmess, full=full)
        assert ap.T == len(sch.steps) and list(ap.aoff) == list(sch.plan["atom_off"])
    atoms_all = np.asarray(sch.plan["atoms_all"])
    aoff = sch.plan["atom_off"]
    assert len(atoms_all) == aoff[-1]
    for t, st in enumerate(sch.steps):
        assert atoms_all[aoff[t]:aoff[t + 1]].tolist() == list(st["atoms"]), t


def test_row_masks_of_the_two_forms_are_the_hash_at_their_sites():
    """atom_row_masks against ggpm_dropout's counter layout: one call at site 0 over the rows of all steps (step t's row j is
    row aoff[t] + j), keeping about 1 - p.  (The name dates from when a full-level form drew one call per step at site t.)"""
    from dropout_masks import atom_row_masks
    from golden_utils import dropout_keep
    aoff, H, p, seed = [0, 5, 5, 12, 40], 16, 0.1, (11, 22)
    c = atom_row_masks(aoff, H, p, seed)
    whole = dropout_keep(40, H, p, 11, 22, 0)
    for t in range(4):
        assert c[t].shape == (aoff[t + 1] - aoff[t], H)
        assert np.array_equal(c[t] > 0, whole[aoff[t]:aoff[t + 1]])
    assert abs(float((np.concatenate(c) > 0).mean()) - (1 - p)) < 0.05
