"""GPU: the tree-only models 'prop' / 'prop-opt' against the reference's own steps (tests/golden/motif_vae), in both forms
of the decoder's level, and the attachment-head kernel (csrc/motif_assm.hip) against a torch restatement."""
import numpy as np
import pytest
import torch

from motif_fixtures import MotifGolden, assm_head_reference, head_case as _head_case, names

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = names()


def _step(g, model, batch, beta=None):
    tensors, sch, orders, homos, lumos = batch
    out = model(None, None, tensors, orders, homos, lumos, beta=g.beta if beta is None else beta, perturb_z=False,
                schedule=sch)
    out[0].backward()
    return out


FORMS = ["driver", "opbyop", "stepwise"]


def _set_form(monkeypatch, form):
    """The decoder's three forms: the level as one tree-level driver call per direction (default), op by op, or the
    reference's step loop; -> list that records every driver call."""
    from ggpm_amd import _dev
    from ggpm_amd import tree_decode as TD
    monkeypatch.setattr(_dev, "DECODER_BATCHED", form != "stepwise")
    monkeypatch.setattr(_dev, "TREE_DRIVER", form == "driver")
    calls, real = [], TD.tree_level

    def spy(*a, **k):
        calls.append(a[3] is None)          # (lin_seq None: the embedding-input mode)
        return real(*a, **k)
    monkeypatch.setattr(TD, "tree_level", spy)
    return calls


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES)
def test_step_matches_reference(name, form, monkeypatch):
    calls = _set_form(monkeypatch, form)
    g = MotifGolden(name)
    model = g.model().to(DEV)
    out = _step(g, model, g.batch())
    assert calls == ([True] if form == "driver" else []), (form, calls)
    if g.kind == "prop-opt":
        assert not bool(out[2])
    g.check_step(model, out[0].detach().cpu(), out[1])


def test_reference_call_shape_and_schedule_ahead():
    """``model(*batch, beta=beta)`` with the networkx graphs, and through ScheduleAhead: the fixture's step both ways."""
    from ggpm_amd import synth
    from ggpm_amd.dataloader import ScheduleAhead
    g = MotifGolden("prop_lstm_s61")
    specs = g.specs()
    mols, graphs, tensors, orders, _, _ = synth.train_batch(specs)
    batch = (mols, graphs, tensors, orders, g.z["t_homo"], g.z["t_lumo"])
    for wrap in (False, True):
        model = g.model().to(DEV)
        it = ScheduleAhead([batch], model) if wrap else [batch]
        for b in it:
            loss, metrics = model(*b, beta=g.beta, perturb_z=False)
            loss.backward()
        g.check_step(model, loss.detach().cpu(), metrics)


@pytest.mark.parametrize("name", ["prop_gru_s60", "propopt_lstm_s64"])
def test_two_steps_bitwise_equal(name):
    g = MotifGolden(name)
    res = []
    for _ in range(2):
        model = g.model().to(DEV)
        out = _step(g, model, g.batch())
        res.append([out[0].detach().cpu().double()] +
                   [p.grad.detach().cpu().clone() for p in model.parameters() if p.grad is not None])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_backward_adds_into_existing_grad():
    g = MotifGolden("prop_gru_s60")
    model = g.model().to(DEV)
    batch = g.batch()
    _step(g, model, batch)
    first = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    _step(g, model, batch)
    for k, p in model.named_parameters():
        if k in first:
            assert torch.allclose(p.grad, 2 * first[k], rtol=1e-5, atol=1e-7), k


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("H,L", [(16, 16), (250, 24), (300, 56)])
def test_head_kernel_matches_oracle(H, L, distinct):
    """Singles, pairs, a prediction with n == max_cls_size (no pad row), pad rows; rows equal or not (dropout)."""
    from ggpm_amd.motif_decoder import _MotifAssm
    C, B = 6, 3
    preds = [(2, 1, 3, 0), (3, 2, 0, 2), (6, 1, 19, 1), (1, 2, 5, 0), (6, 2, 7, 2), (4, 1, 0, 1)]
    rows, meta, W1, b1, Wa, ba, z, n_cand = _head_case(H + L, H, L, C, preds, B, distinct)
    ref = [t.double().requires_grad_(True) for t in (rows, z, W1, b1, Wa, ba)]
    loss_r, acc_r = assm_head_reference(ref[0], meta, C, ref[2], ref[3], ref[4], ref[5], ref[1])
    loss_r.backward()
    dv = [t.to(DEV).requires_grad_(True) for t in (rows, z, W1, b1, Wa, ba)]
    loss, acc = _MotifAssm.apply(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], meta.to(DEV), len(preds), C, n_cand)
    (loss * 1.5).backward()
    assert abs(float(loss) - float(loss_r)) <= 1e-4 * max(1.0, abs(float(loss_r)))
    assert float(acc) == float(acc_r)
    for name, a, r in zip(("rows", "z", "W1", "b1", "Wa", "ba"), dv, ref):
        want = 1.5 * r.grad.numpy()
        got = a.grad.detach().cpu().double().numpy()
        scale = max(np.abs(want).max(), 1e-3)
        if name == "ba":        # analytically zero (the softmax gradients of a prediction sum to 0): rounding noise only
            assert np.abs(got).max() <= 1e-5, (name, np.abs(got).max())
            continue
        assert np.abs(got - want).max() <= 1e-4 * scale, (name, np.abs(got - want).max(), scale)


# ---------------------------------------------------------------------------------------------- dropout 0.1 vs the oracle
P_DROP = 0.1


def _inject_columns(model, H):
    """Every nn.Dropout of the model replaced by a dropout_masks.InjectedDropout with a per-column mask of its own (a shared
    module -- tied embeddings -- stays shared) -> {module id: cols}."""
    import dropout_masks as dm
    from golden_utils import dropout_keep
    Hp = dm.padded(H)
    made, k = {}, 0
    for name, mod in list(model.named_modules()):
        for cname, child in list(mod.named_children()):
            if type(child) is torch.nn.Dropout and not name.startswith("property_optim"):
                if id(child) not in made:
                    k += 1
                    cols = torch.from_numpy(dm.scaled(dropout_keep(1, Hp, P_DROP, 2718281, 3141592, 200 + k)[0], P_DROP))
                    made[id(child)] = dm.InjectedDropout(P_DROP, cols.to(DEV))
                setattr(mod, cname, made[id(child)])
    return {id(m): m.cols.cpu() for m in made.values()}


@pytest.mark.parametrize("form", ["opbyop", "stepwise"])
@pytest.mark.parametrize("name", ["prop_gru_s60", "prop_lstm_s61", "prop_gru_noassm"])
def test_step_with_dropout_matches_oracle(name, form, monkeypatch):
    """Dropout 0.1 at every nn.Dropout of PropertyVAE (the embeddings, the decoder level's E_c / W_o, E_assm through the
    attachment head, the score heads) against tests/motif_oracle.py under the same masks."""
    import motif_oracle as mo
    calls = _set_form(monkeypatch, form)
    g = MotifGolden(name)
    model = g.model(dropout=P_DROP).to(DEV)
    _inject_columns(model, g.H)
    model.train()
    out = _step(g, model, g.batch())
    assert calls == []                      # (dropout active: the driver form is not taken)
    dec = model.decoder
    site_mod = {"encoder.E_c": model.encoder.E_c[1], "encoder.E_i": model.encoder.E_i[1], "decoder.E_c": dec.hmpn.E_c[1],
                "decoder.W_o": dec.hmpn.tree_encoder.W_o[2], "decoder.E_assm": dec.E_assm[1], "topoNN.2": dec.topoNN[2],
                "clsNN.2": dec.clsNN[2], "iclsNN.2": dec.iclsNN[2]}
    assert all(m.calls > 0 for k, m in site_mod.items() if k != "decoder.E_assm" or g.z["ref_assm_batch"].size)

    def drop(site, x, step):
        return x * site_mod[site].cols[:x.shape[-1]].cpu().to(x.dtype)
    ref = g.model(dropout=P_DROP)
    loss_r, metrics_r, grads_r = mo.run(g, torch.float64, drop=drop, model=ref)
    assert abs(float(out[0]) - float(loss_r)) <= 1e-4 * max(1.0, abs(float(loss_r)))
    for k, v in metrics_r.items():
        assert abs(float(out[1][k]) - v) <= 1e-4 * max(1.0, abs(v)), (k, float(out[1][k]), v)
    params = model.state_dict(keep_vars=True)
    for k, gr in grads_r.items():
        mine = params[k].grad
        if gr is None:
            assert mine is None or float(mine.abs().max()) == 0.0, k
            continue
        want = gr.numpy()
        got = mine.detach().double().cpu().numpy()
        scale = np.abs(want).max()
        if scale < 1e-6 or k.endswith("W_assm.bias"):
            assert np.abs(got).max() < 1e-4, k
            continue
        assert np.abs(got - want).max() <= 1e-4 * scale, (k, np.abs(got - want).max() / scale)
