"""GPU: full training steps with dropout 0.1 (ten of the reference's shipped configs, both ``*_hier_*`` fine-tune configs
among them) against the oracle under the same masks -- the VAE step in every form of the decoder, at config shapes, and
the HierPropOptVAE fine-tune step.  tests/dropout_masks.py says which masks: the HIP code's own (encoder drivers, the
atom level's W_o, the property heads) restated from pinned seeds; test-owned per-column masks at torch's nn.Dropout
modules (tree-side levels, E_assm, score heads, the atom level's W_o in the step-by-step forms)."""
import types

import numpy as np
import pytest
import torch

import dropout_masks as dm
import property_fixtures as pf
import property_oracle as po
from golden_utils import VaeGolden, dropout_keep, vae_case_names

pytestmark = pytest.mark.gpu

TOL = 1e-4
P = 0.1
ENC_SEED = (123456789, 987654321)
ATOM_SEED = (24681357, 97531)
HEAD_SEED = (12345, 678)


def _dev():
    return torch.device("cuda:0")


def _set_mode(monkeypatch, mode):
    """The forms of the decoder (ggpm_amd/_dev.py), as tests/test_gpu_parity.py::test_vae_step_matches_reference_golden
    selects them."""
    from ggpm_amd import _dev as dev_settings
    monkeypatch.setattr(dev_settings, "DECODER_BATCHED", mode != "stepwise")
    monkeypatch.setattr(dev_settings, "ATOM_DECODE", mode.startswith("batched"))
    monkeypatch.setattr(dev_settings, "ATOM_AHEAD", mode == "batched")
    if mode == "batched_opheads":
        monkeypatch.setattr(dev_settings, "HEADS_COMPOSITE", False)


def _mode_cases():
    names = vae_case_names()
    picked = [next((n for n in names if cell in n), None) for cell in ("gru", "lstm")]
    others = ["batched_inline", "batched_opheads", "levels", "stepwise"]
    return [(n, "batched") for n in names] + [(n, m) for n in picked if n for m in others]


def _model(cls, args, sd, pin=True):
    """``cls(args)`` on the GPU with the weights ``sd``, in training mode; ``pin``: the HIP mask seeds pinned and the
    decoder's nn.Dropout modules replaced (-> (model, {module path: InjectedDropout}))."""
    model = cls(args).to(_dev())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys
    assert all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.")) for k in res.missing_keys), res.missing_keys
    model.train()
    inj = {}
    if pin:
        model.encoder._dropout_seed = ENC_SEED
        model.decoder.hmpn.graph_encoder._dropout_seed = ATOM_SEED
        if hasattr(model, "property_optim"):
            model.property_optim._dropout_seed = HEAD_SEED
        inj = dm.inject(model.decoder, args.dropout, args.hidden_size)
    return model, inj


def _oracle_params(sd, tie, dtype=torch.float32):
    p = {k: torch.from_numpy(v).to(dtype if v.dtype == np.float32 else torch.float64).requires_grad_(True)
         for k, v in sd.items()}
    if tie:
        for k in ("E_c.0.weight", "E_i.0.weight"):
            p["encoder." + k] = p["decoder.hmpn." + k]
    return p


def _oracle_drop(H, sch, tt, gt, mode, counts=None):
    """(encoder masks, decoder drop) of the form ``mode``: the atom level's W_o is the HIP hash in the ATOM_DECODE forms
    (site 0 over all steps' rows), the injected module in ``levels`` / ``stepwise``."""
    atom_rows = None
    if mode.startswith("batched"):
        atom_rows = dm.atom_row_masks(sch.plan["atom_off"], H, P, ATOM_SEED)
    return (dm.encoder_masks(tt[0].shape[0], gt[0].shape[0], H, P, ENC_SEED),
            dm.oracle_drop(H, P, atom_rows, counts))


def _check_sites(inj, counts, mode):
    """Which injected modules the step called, and over how many rows: a form that skips a site, or masks rows the
    reference does not, fails here."""
    want = {}
    for site, n in counts.items():
        if site == "graph_encoder.W_o" and mode.startswith("batched"):
            continue                                     # the HIP hash path's own masks, not the module
        want[dm.COLUMN_SITES[site]] = want.get(dm.COLUMN_SITES[site], 0) + n
    for path, m in inj.items():
        if path == "hmpn.graph_encoder.W_o.2" and mode.startswith("batched"):
            assert m.calls == 0, "%s: the atom level's W_o reached the nn.Dropout module in form %s" % (path, mode)
            continue
        assert m.calls > 0, "%s: never called in form %s" % (path, mode)
        assert m.rows == want[path], "%s: %d rows masked, the reference masks %d" % (path, m.rows, want[path])


def _compare_grads(named, p32, fp64_grads, what=""):
    """Every parameter gradient within TOL of the oracle's fp32 run or -- where a ReLU kink falls on the other side in
    fp32 vs fp64 (see test_gpu_parity.py::test_vae_step_at_config_shapes_matches_oracle) -- of its fp64 run."""
    gmax = max(float(v.grad.abs().max()) for v in p32.values() if v.grad is not None)
    p64 = None
    for k, v in named:
        want = p32[k].grad.double().numpy() if p32[k].grad is not None else np.zeros(tuple(v.shape))
        got = v.grad.double().cpu().numpy() if v.grad is not None else np.zeros_like(want)
        scale = float(np.abs(want).max())
        if scale <= 1e-6 * gmax:
            assert float(np.abs(got).max()) <= 1e-4 * gmax, (what, k)
            continue
        e32 = float(np.abs(got - want).max()) / scale
        if e32 < TOL:
            continue
        if p64 is None:
            p64 = fp64_grads()
        w64 = p64[k].grad.numpy()
        e64 = float(np.abs(got - w64).max()) / float(np.abs(w64).max())
        split = float(np.abs(want - w64).max()) / float(np.abs(w64).max())
        assert split > TOL and e64 < TOL, (what, k, "HIP vs the oracle's fp32 run %.2e, vs its fp64 run %.2e; fp32 vs "
                                           "fp64 %.2e" % (e32, e64, split))


def _vae_step_vs_oracle(args, sd, specs, beta, mode, tie):
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropertyVAE
    from oracle import ref_encoder as ref, ref_decoder as refd
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    B, H = len(specs), args.hidden_size
    model, inj = _model(HierPropertyVAE, args, sd)
    loss, metrics = model(None, None, tensors, [None] * B, None, None, beta=beta, perturb_z=False, schedule=sch)
    loss.backward()
    tt, gt = ref.to_long_tensors(tensors[0]), ref.to_long_tensors(tensors[1])
    voc_mask = args.vocab.mask

    def oracle(dtype, counts=None):
        p = _oracle_params(sd, tie, dtype)
        masks, drop = _oracle_drop(H, sch, tt, gt, mode, counts)
        rl, rkl, accs, _ = refd.vae_forward(p, args.rnn_type, args.depthT, args.depthG, args.diterT, args.diterG, tt, gt,
                                            sch, voc_mask.to(dtype), beta, masks=masks, drop=drop)
        rl.backward()
        return p, rl, rkl, accs

    counts = {}
    p, rl, rkl, accs = oracle(torch.float32, counts)
    _check_sites(inj, counts, mode)
    assert abs(float(loss.detach()) - float(rl.detach())) <= TOL * abs(float(rl.detach()))
    assert abs(metrics["KL:"] - float(rkl.detach())) <= TOL * max(1.0, abs(float(rkl.detach())))
    assert np.allclose([metrics[k] for k in ("Word", "I-Word", "Topo", "Assm")], [float(x) for x in accs], atol=1e-6)
    _compare_grads(list(model.named_parameters()), p, lambda: oracle(torch.float64)[0], mode)
    return model, loss


@pytest.mark.parametrize("name,mode", _mode_cases())
def test_vae_step_with_dropout_matches_oracle(name, mode, monkeypatch):
    """HierPropertyVAE's training step at p = 0.1 (perturb_z=False) on the vae_* fixtures' models, in every form of the
    decoder: loss, KL, the four accuracies and every parameter gradient against the oracle under the same masks."""
    from ggpm_amd.vocab import IndexPairVocab
    _set_mode(monkeypatch, mode)
    g = VaeGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.dropout = P
    _vae_step_vs_oracle(args, g.state_dict(), g.specs(), g.beta, mode, g.tie)


@pytest.mark.parametrize("rnn,H,L,depth,B,motifs,vocab,tie,seed", [
    ("GRU", 300, 32, 20, 32, (8, 12), (500, 1500), False, 4242),      # configs[1]
    ("LSTM", 250, 24, 20, 20, (6, 14), (721, 6489), False, 77),       # configs[0]: 9 attachments per motif
    ("LSTM", 600, 24, 20, 8, (6, 14), (721, 6489), True, 79),         # configs[3]'s model: H=600, tied embeddings
])
def test_vae_step_with_dropout_at_config_shapes_matches_oracle(rnn, H, L, depth, B, motifs, vocab, tie, seed):
    """The same comparison at the model shapes of BASELINE.json's configs, default form of the decoder."""
    from ggpm_amd import synth
    from ggpm_amd.params import vae_param_shapes, tied_state_dict, seeded_state_dict
    from ggpm_amd.vocab import IndexPairVocab
    n_motif, n_attach = vocab
    specs = synth.random_batch(seed, B, motifs=motifs, n_motif_vocab=n_motif, n_attach_vocab=n_attach)
    sd = seeded_state_dict(vae_param_shapes(rnn, H, L, n_motif, n_attach), seed)
    if tie:
        sd = tied_state_dict(sd)
    args = types.SimpleNamespace(vocab=IndexPairVocab(n_motif, n_attach), rnn_type=rnn, embed_size=H, hidden_size=H,
                                 atom_vocab=types.SimpleNamespace(size=lambda: 38), depthT=depth, depthG=depth, diterT=1,
                                 diterG=5, dropout=P, latent_size=L, tie_embedding=tie)
    _vae_step_vs_oracle(args, sd, specs, 0.1, "batched", tie)


@pytest.mark.parametrize("name", pf.names("propopt"))
def test_propopt_step_with_dropout_matches_oracle(name):
    """HierPropOptVAE's fine-tune step at p = 0.1 (the *_hier_* configs) on the propopt_* fixtures' models: the oracle's
    encoder and decoder under the same masks, the heads' restatement (property_oracle.heads_step) with the heads' masks,
    the heads' d(latent) fed into the oracle's latent vector.  Total, recon, HOMO and LUMO MSE and every gradient
    (LossWeigh's fp64 log-variances included: propopt_gru_s52 has loss_scaling)."""
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropOptVAE
    from ggpm_amd.vocab import IndexPairVocab
    from oracle import ref_encoder as ref, ref_decoder as refd
    g = pf.PropOptGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.dropout = P
    specs = g.specs()
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    sd = g.state_dict()
    t_h, t_l = g.z["t_homo"], g.z["t_lumo"]
    model, inj = _model(HierPropOptVAE, args, sd)
    total, metrics, clipped = model(None, None, tensors, [None] * g.B, t_h.tolist(), t_l.tolist(), beta=0.1,
                                    perturb_z=False, schedule=sch)
    total.sum().backward()
    assert not bool(clipped)
    tt, gt = ref.to_long_tensors(tensors[0]), ref.to_long_tensors(tensors[1])
    half, H = g.latent // 2, g.H
    homo, lumo = po.head_layers(sd, "property_optim.homo_linear"), po.head_layers(sd, "property_optim.lumo_linear")
    lv = {k: float(sd["loss_weigh.%s_log_var" % k][0]) if g.scaling else 0.0 for k in ("recon", "homo", "lumo")}
    w = {k: float(np.exp(-v)) for k, v in lv.items()}

    def oracle(dtype, counts=None):
        p = _oracle_params(sd, g.tie, dtype)
        masks, drop = _oracle_drop(H, sch, tt, gt, "batched", counts)
        cap = {}

        def latent(z):
            cap["z"] = z
            return z
        _, _, accs, recon = refd.vae_forward(p, g.rnn, g.depthT, g.depthG, g.diterT, g.diterG, tt, gt, sch,
                                             args.vocab.mask.to(dtype), 0.0, masks=masks, drop=drop, latent=latent)
        z = cap["z"]
        hs = po.heads_step(homo, lumo, z.detach().double().numpy(), half, t_h.astype(np.float64),
                           t_l.astype(np.float64), p=P, seed=HEAD_SEED, dloss=(w["homo"], w["lumo"]))
        torch.autograd.backward([recon, z], [torch.tensor(w["recon"], dtype=recon.dtype),
                                             torch.from_numpy(hs["dz"]).to(z.dtype)])
        return p, recon, hs, accs

    counts = {}
    p, recon, hs, accs = oracle(torch.float32, counts)
    _check_sites(inj, counts, "batched")
    r = float(recon.detach()) * w["recon"] + lv["recon"]
    mh = hs["loss"][0] * w["homo"] + lv["homo"]
    ml = hs["loss"][1] * w["lumo"] + lv["lumo"]
    for key, want in (("Recs_Loss", r), ("HOMO_MSE", mh), ("LUMO_MSE", ml), ("Loss", r + mh + ml)):
        assert abs(metrics[key] - want) <= TOL * max(1.0, abs(want)), (key, metrics[key], want)
    assert abs(float(total.detach().reshape(-1)[0]) - (r + mh + ml)) <= TOL * max(1.0, abs(r + mh + ml))
    assert np.allclose([metrics[k] for k in ("Word", "I-Word", "Topo", "Assm")], [float(x) for x in accs], atol=1e-6)
    # the heads and LossWeigh against the restatement (fp64), the rest against the oracle's autograd
    opt = model.property_optim
    heads = {}
    for hi, head in enumerate((opt.homo_linear, opt.lumo_linear)):
        for i, lin in enumerate(head.linears()):
            heads[id(lin.weight)], heads[id(lin.bias)] = hs["grads"][hi][i]
    for k, v in model.named_parameters():
        if id(v) in heads:
            want = heads[id(v)]
            got = v.grad.double().cpu().numpy()
            assert np.abs(got - want).max() <= TOL * max(np.abs(want).max(), 1e-12), k
    if g.scaling:
        L = {"recon": float(recon.detach()), "homo": hs["loss"][0], "lumo": hs["loss"][1]}
        for k in ("recon", "homo", "lumo"):
            got = float(getattr(model.loss_weigh, k + "_log_var").grad[0])
            want = 1.0 - L[k] * w[k]
            assert abs(got - want) <= TOL * max(1.0, abs(want)), (k, got, want)
    rest = [(k, v) for k, v in model.named_parameters() if id(v) not in heads and not k.startswith("loss_weigh.")]
    assert model.R_var.weight.grad is None and model.R_var.bias.grad is None
    for k, v in rest:
        if p[k].grad is None:          # (R_var; the tree encoder's W_o: None in the reference, None or zero here)
            assert v.grad is None or not bool(v.grad.ne(0).any()), k
    _compare_grads([(k, v) for k, v in rest if p[k].grad is not None], p, lambda: oracle(torch.float64)[0], name)


# ------------------------------------------------------------------------------------------------- sanity checks
def _fixture_step(name, dropout, seeds=None, train=True, atom_seed=ATOM_SEED):
    """One VAE step on fixture ``name`` with dropout ``dropout`` -> (loss, {parameter: grad})."""
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropertyVAE
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.dropout = dropout
    specs = g.specs()
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    model, _ = _model(HierPropertyVAE, args, g.state_dict(), pin=False)
    model.encoder._dropout_seed = ENC_SEED
    model.decoder.hmpn.graph_encoder._dropout_seed = atom_seed
    if not train:
        model.eval()
    torch.manual_seed(5)            # (the torch modules' masks; the HIP ones come from the pinned seeds)
    loss, _ = model(None, None, tensors, [None] * g.B, None, None, beta=g.beta, perturb_z=False, schedule=sch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}


@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s41"])
def test_dropout_eval_mode_seeds_and_reproducibility(name):
    """Eval mode with p = 0.1 is bit-identical to p = 0; two atom-level seeds give different losses; two runs with the
    same seeds give bit-identical loss and gradients."""
    ev = _fixture_step(name, P, train=False)
    nodrop = _fixture_step(name, 0.0)
    assert torch.equal(ev[0], nodrop[0])
    assert set(ev[1]) == set(nodrop[1])
    for k in ev[1]:
        assert torch.equal(ev[1][k], nodrop[1][k]), k
    a = _fixture_step(name, P)
    b = _fixture_step(name, P)
    other = _fixture_step(name, P, atom_seed=(ATOM_SEED[0] + 1, ATOM_SEED[1]))
    assert not torch.equal(a[0], nodrop[0])
    assert not torch.equal(a[0], other[0])
    assert torch.equal(a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_atom_level_mask_keeps_about_1_minus_p_and_leaves_the_pad_columns():
    """ggpm_dropout as the atom level calls it (rows of all steps, H columns of an Hp-wide buffer, site 0) on ones: the
    restated mask exactly, scaled by 1 / (1 - p), the pad columns untouched, and a keep fraction of 0.9 +- 0.02."""
    from ggpm_amd import _lib
    g = VaeGolden("vae_lstm_s43")
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd import synth
    specs = g.specs()
    sch = DecodeSchedule.from_specs(specs, synth.tensorize(specs))
    rows, H = sch.plan["atom_off"][-1], g.H
    Hp = dm.padded(H)
    x = torch.ones(rows, Hp, dtype=torch.float32, device=_dev())
    lib = _lib.load()
    _lib.check(lib.ggpm_dropout(x.data_ptr(), rows, H, Hp, P, ATOM_SEED[0], ATOM_SEED[1], 0, None), "dropout")
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    keep = dropout_keep(rows, H, P, ATOM_SEED[0], ATOM_SEED[1], 0)
    assert np.array_equal(got[:, :H] > 0, keep)
    assert np.allclose(got[:, :H][keep], 1.0 / (1.0 - P), rtol=1e-6)
    assert np.array_equal(got[:, H:], np.ones((rows, Hp - H), np.float32))
    assert abs(float(keep.mean()) - (1 - P)) <= 0.02, float(keep.mean())
