"""GPU: the forward-only forms (no-grad / inference-mode calls) against the training forward of the same model: bit-identical
outputs, a fraction of the memory, no state carried into the next training step; the public no-grad entry points
(predict_properties, PropertyVAEOptimizer.optimize) against the numpy oracle."""
import ctypes

import numpy as np
import pytest
import torch

import property_oracle as po
from golden_utils import VaeGolden, assert_close
from motif_fixtures import MotifGolden
import property_fixtures as pf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["no_grad", "inference_mode"]


def _ctx(mode):
    return {"grad": torch.enable_grad, "no_grad": torch.no_grad, "inference_mode": torch.inference_mode}[mode]()


def _values(out):
    """Every tensor / number of a model's output, flattened in order (metrics read by key)."""
    vals = []
    for o in out if isinstance(out, (tuple, list)) else (out,):
        if isinstance(o, torch.Tensor):
            vals.append(o.detach().clone())
        elif isinstance(o, dict):
            vals.extend(float(o[k]) for k in sorted(o.keys()))
        elif isinstance(o, (tuple, list)):
            vals.extend(_values(o))
        else:
            vals.append(float(bool(o)))
    return vals


def _equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y), (i, (x - y).abs().max() if x.shape == y.shape else (x.shape, y.shape))
        else:
            assert x == y or (x != x and y != y), (i, x, y)


def _hier(kind, name, dropout=0.0):
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropertyVAE, HierPropOptVAE
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name) if kind == "hier-prop" else pf.PropOptGolden(name)
    args = g.args(IndexPairVocab(g.n_motif, g.n_attach))
    args.dropout = dropout
    model = (HierPropertyVAE if kind == "hier-prop" else HierPropOptVAE)(args).to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=False)
    specs = g.specs()
    tensors = synth.tensorize(specs)
    sch = DecodeSchedule.from_specs(specs, tensors)
    if kind == "hier-prop":
        homos = lumos = None
    else:
        homos, lumos = g.z["t_homo"].tolist(), g.z["t_lumo"].tolist()
    return model, (None, None, tensors, [None] * g.B, homos, lumos), sch, g


def _motif(name):
    g = MotifGolden(name)
    tensors, sch, orders, homos, lumos = g.batch()
    return g.model().to(DEV), (None, None, tensors, orders, homos, lumos), sch, g


def _forward(model, batch, sch, mode, seed=5):
    torch.manual_seed(seed)             # (the decoder's torch Dropout modules; the HIP masks come from pinned seeds)
    with _ctx(mode):
        out = model(*batch, beta=0.1, perturb_z=False, schedule=sch)
    torch.cuda.synchronize()
    return _values(out)


CASES = [("hier-prop", "vae_gru_s42"), ("hier-prop", "vae_lstm_s41")] + \
        [("hier-prop-opt", n) for n in pf.names("propopt")] + [("motif", "prop_gru_s60"), ("motif", "propopt_lstm_s64")]


@pytest.mark.parametrize("kind,name", CASES)
def test_eval_forward_is_bit_identical_without_grad(kind, name):
    model, batch, sch, g = _motif(name) if kind == "motif" else _hier(kind, name)
    model.eval()
    ref = _forward(model, batch, sch, "grad")
    for mode in MODES:
        _equal(_forward(model, batch, sch, mode), ref)


def test_hier_prop_opt_cases_cover_loss_scaling_on_and_off():
    assert {pf.PropOptGolden(n).scaling for n in pf.names("propopt")} == {False, True}


# the decoder's other forms (ggpm_amd/_dev.py): no worker thread, tree-side levels as the Python composite
FORMS = {"no_worker": dict(ATOM_ASYNC=False), "tree_composite": dict(TREE_DRIVER=False)}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s41"])
def test_decoder_forms_are_bit_identical_without_grad(name, form, monkeypatch):
    from ggpm_amd import _dev
    for k, v in FORMS[form].items():
        monkeypatch.setattr(_dev, k, v)
    model, batch, sch, _ = _hier("hier-prop", name)
    model.eval()
    ref = _forward(model, batch, sch, "grad")
    for mode in MODES:
        _equal(_forward(model, batch, sch, mode), ref)


def test_no_grad_forward_joins_the_decode_worker():
    """Nothing of a no-grad forward waits for a backward: no pending read-out, no buffers held for the worker."""
    from ggpm_amd import _dev, atom_decode
    assert _dev.ATOM_ASYNC
    model, batch, sch, _ = _hier("hier-prop", "vae_gru_s42")
    model.eval()
    for mode in MODES:
        with _ctx(mode):
            model(*batch, beta=0.1, perturb_z=False, schedule=sch)
        assert not atom_decode._INFLIGHT and not hasattr(atom_decode, "_PENDING"), mode


@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s41"])
def test_train_mode_dropout_forward_is_bit_identical_without_grad(name):
    model, batch, sch, _ = _hier("hier-prop", name, dropout=0.1)
    model.train()
    model.encoder._dropout_seed = (123456789, 987654321)
    model.decoder.hmpn.graph_encoder._dropout_seed = (24681357, 97531)
    ref = _forward(model, batch, sch, "grad")
    for mode in MODES:
        _equal(_forward(model, batch, sch, mode), ref)


def _encoder_vae(rnn, H, depth, latent=32):
    from ggpm_amd.property_vae import HierEncoderVAE
    from ggpm_amd.vocab import IndexPairVocab

    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = rnn, H, H, depth, depth
    a.dropout, a.latent_size = 0.0, latent
    torch.manual_seed(0)
    return HierEncoderVAE(a).to(DEV).eval()


def _synth_tensors(B, motifs, seed=1000):
    from ggpm_amd import synth
    from ggpm_amd.property_vae import make_cuda
    return make_cuda(synth.tensorize(synth.random_batch(seed, B, motifs=motifs, n_motif_vocab=500, n_attach_vocab=1500)))


@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_bf16_encoder_forward_is_bit_identical_without_grad(rnn):
    """Gate dtype bf16 on an atom level large enough for bf16 storage (configs[4] molecules): the forward-only form keeps
    the depth loop's bf16 roundings."""
    from ggpm_amd import _lib
    model = _encoder_vae(rnn, 600, 6)
    model.encoder.gate_dtype = "bf16"
    tensors = _synth_tensors(16, (46, 58))
    E1 = tensors[1][1].shape[0]
    assert _lib.load().ggpm_level_bf16_storage(E1, 600) == 1, E1
    with torch.enable_grad():
        ref = _values(model(tensors, perturb_z=False))
    for mode in MODES:
        with _ctx(mode):
            _equal(_values(model(tensors, perturb_z=False)), ref)


@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_tree_fixed_point_forward_is_bit_identical_without_grad(rnn):
    """Tree-side levels with depth well above the batch's longest message chain: both forms stop at chain + 1 steps."""
    from ggpm_amd.nnutils import read_hint
    model = _encoder_vae(rnn, 64, 16)
    tensors = _synth_tensors(8, (8, 12))
    chain = read_hint(tensors[0][3], "ggpm_chain", 0)
    assert 0 < chain and chain + 1 < 16, chain
    with torch.enable_grad():
        ref = _values(model(tensors, perturb_z=False))
    for mode in MODES:
        with _ctx(mode):
            _equal(_values(model(tensors, perturb_z=False)), ref)


def test_encoder_no_grad_memory_is_an_eighth_of_the_saved_arena():
    from ggpm_amd import _lib, fused
    from ggpm_amd.encoder import _RING
    model = _encoder_vae("GRU", 300, 20)
    tree, graph = _synth_tensors(32, (8, 12))
    roots = _RING.upload([st for st, _ in tree[-1]], DEV)
    enc = model.encoder
    with torch.no_grad():
        enc.forward_padded(tree, graph, roots=roots)          # warm-up: caches, packed parameter list
    torch.cuda.synchronize()
    dims = fused.EncDims(300, 300, 20, 20, 38, 500, 1500, graph[0].shape[0], graph[1].shape[0], graph[2].shape[1],
                         graph[3].shape[1], tree[0].shape[0], tree[1].shape[0], tree[2].shape[1], tree[3].shape[1],
                         tree[4].shape[1], 32, 0, 0, 0.0, 0, 0, 0)
    saved = int(_lib.load().ggpm_encoder_saved_bytes(ctypes.byref(dims)))
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        out = enc.forward_padded(tree, graph, roots=roots)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < saved / 8, (peak, saved)
    del out


def _configs1_vae():
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropertyVAE
    from ggpm_amd.vocab import IndexPairVocab

    class A:
        pass
    a = A()
    a.vocab, a.atom_vocab = IndexPairVocab(500, 1500), type("V", (), {"size": lambda s: 38})()
    a.rnn_type, a.embed_size, a.hidden_size, a.depthT, a.depthG = "GRU", 300, 300, 20, 20
    a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = 1, 5, 0.0, 32, False
    torch.manual_seed(0)
    model = HierPropertyVAE(a).to(DEV).eval()
    specs = synth.random_batch(1000, 32, motifs=(8, 12), n_motif_vocab=500, n_attach_vocab=1500)
    tensors = synth.tensorize(specs)
    return model, (None, None, tensors, [None] * 32, None, None), DecodeSchedule.from_specs(specs, tensors)


def _peak(model, batch, sch, mode):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with _ctx(mode):
        out = model(*batch, beta=0.1, perturb_z=False, schedule=sch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_vae_no_grad_forward_peaks_at_half_the_grad_forward():
    model, batch, sch = _configs1_vae()
    _peak(model, batch, sch, "no_grad")                       # warm-up
    grad = _peak(model, batch, sch, "grad")
    nograd = _peak(model, batch, sch, "no_grad")
    assert nograd * 2 <= grad, (nograd, grad)


@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s41"])
def test_no_grad_forward_between_training_steps_leaves_no_state(name):
    from ggpm_amd import _dev
    assert _dev.ATOM_ASYNC and _dev.ATOM_AHEAD
    model, batch, sch, _ = _hier("hier-prop", name)
    model.eval()

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = model(*batch, beta=0.1, perturb_z=False, schedule=sch)
        loss.backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    step()
    plain = step()
    step()
    with torch.no_grad():
        model(*batch, beta=0.1, perturb_z=False, schedule=sch)
    after = step()
    with torch.inference_mode():
        model(*batch, beta=0.1, perturb_z=False, schedule=sch)
    again = step()
    assert set(plain) == set(again)
    for k in plain:
        assert torch.equal(plain[k], again[k]), k
    assert set(plain) == set(after)
    for k in plain:
        assert torch.equal(plain[k], after[k]), k


@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s41"])
def test_two_atom_levels_in_flight_travel_with_their_own_handles(name):
    """Two atom levels issued ahead, of two schedules of the same batch, joined in the other order: each handle carries
    its own run, so both steps give the bits of an ordinary step, and nothing stays with the decode worker."""
    from ggpm_amd import _dev, atom_decode
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import make_cuda, rsample
    assert _dev.ATOM_ASYNC and _dev.ATOM_AHEAD
    model, batch, sch_a, g = _hier("hier-prop", name)
    sch_b = DecodeSchedule.from_specs(g.specs(), batch[2])
    model.train()                                               # (dropout 0)

    def grads(loss):
        model.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    ref = {id(s): grads(model(*batch, beta=0.1, perturb_z=False, schedule=s)[0]) for s in (sch_a, sch_b)}

    tensors = make_cuda(batch[2])
    ahead = {id(s): model.decoder.start_atom_level(s, tensors) for s in (sch_a, sch_b)}
    assert ahead[id(sch_a)] is not None and ahead[id(sch_b)] is not None
    for s in (sch_b, sch_a):
        root = model.encoder.forward_padded(*tensors, beside=True)[0]
        root, kl = rsample(root, model.R_mean, model.R_var, False)
        loss = model.decoder(None, (root, root, root), None, tensors, batch[3], schedule=s, atom=ahead[id(s)])[0] + 0.1 * kl
        loss, got = grads(loss)
        assert torch.equal(loss, ref[id(s)][0])
        assert set(got) == set(ref[id(s)][1])
        for k in got:
            assert torch.equal(got[k], ref[id(s)][1][k]), k
    assert not atom_decode._INFLIGHT


def _layers(opt):
    sd = {k: v.detach().cpu().numpy() for k, v in opt.state_dict().items()}
    return po.head_layers(sd, "homo_linear"), po.head_layers(sd, "lumo_linear")


@pytest.mark.parametrize("kind,name", [("hier-prop-opt", "propopt_gru_s50"), ("motif", "propopt_gru_s63")])
def test_predict_properties_matches_the_oracle_on_the_mean_latent(kind, name):
    model, batch, _, _ = _motif(name) if kind == "motif" else _hier(kind, name)
    model.eval()
    homo, lumo = model.predict_properties(batch)
    z, _ = model.encode_latent(batch[2], perturb=False)         # grad-enabled: the training forward's mean latent
    z = z.detach().cpu().numpy().astype(np.float64)
    half = model.latent_size
    layers = _layers(model.property_optim)
    assert_close(homo.cpu().numpy(), po.head_forward(layers[0], z[:, :half])[0], "homo")
    assert_close(lumo.cpu().numpy(), po.head_forward(layers[1], z[:, half:])[0], "lumo")


def test_tree_only_optimizer_matches_the_search_oracle():
    from ggpm_amd.property_control import PropertyVAEOptimizer

    class A:
        optimize_type, property_optim_step, patience, patience_threshold = "fixed", 5, 3, 0.01
        property_delta, latent_lr, max_steps = 0.01, 0.05, 10000
    model, batch, _, _ = _motif("propopt_gru_s63")
    model.eval()
    search = PropertyVAEOptimizer(model, A())
    latent, (ph, pl) = search.optimize(batch)
    z, _ = model.encode_latent(batch[2], perturb=False)
    half = model.latent_size
    homo, lumo = _layers(model.property_optim)
    z_ref, pred_ref, steps_ref, _ = po.search("fixed", homo, lumo, z.detach().cpu().numpy(), half, batch[4], batch[5],
                                              A.latent_lr, A.property_optim_step, A.property_delta, A.patience,
                                              A.patience_threshold, A.max_steps)
    assert (search.steps_taken.cpu().numpy() == steps_ref).all()
    assert_close(latent.cpu().numpy(), z_ref, "latent")
    assert_close(ph.cpu().numpy(), pred_ref[0], "homo")
    assert_close(pl.cpu().numpy(), pred_ref[1], "lumo")
