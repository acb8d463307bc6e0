"""GPU: the property heads (csrc/property.hip) and HierPropOptVAE against the restatement and the reference's fixtures, the
fine-tune loop shape, clip_negative_loss, and the one-launch latent search against the reference's search fixtures."""
import os
import time
import warnings

import numpy as np
import pytest
import torch

import property_fixtures as pf
import property_oracle as po
from golden_utils import assert_close, dropout_keep  # noqa: F401  (dropout_keep: the masks the restatement injects)

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _dev():
    return torch.device("cuda:0")


def _heads(half, hidden, dropout=0.0, seed=0):
    from ggpm_amd.property import PropertyOptimizer
    torch.manual_seed(seed)
    opt = PropertyOptimizer(half, hidden, dropout)
    with torch.no_grad():
        for p in opt.parameters():
            p.normal_(0, 0.4)
    return opt.to(_dev())


def _layers(opt, dtype=np.float64):
    sd = {k: v.detach().cpu().numpy() for k, v in opt.state_dict().items()}
    return po.head_layers(sd, "homo_linear", dtype), po.head_layers(sd, "lumo_linear", dtype)


HEAD_SHAPES = [
    # B, half, hidden
    (1, 12, [64, 64]),
    (20, 12, [64, 64]),
    (320, 12, [64, 64]),
    (20, 5, 7),
    (37, 12, [33, 17, 5]),
    (20, 16, [64, 48, 40, 24]),
    (9, 12, 128),
]


@pytest.mark.parametrize("B,half,hidden", HEAD_SHAPES)
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_heads_forward_backward_match_the_restatement(B, half, hidden, dropout):
    opt = _heads(half, hidden, dropout, seed=B + half)
    opt.train()
    opt._dropout_seed = (12345, 678)
    rs = np.random.RandomState(B)
    z = torch.from_numpy(rs.standard_normal((B, 2 * half)).astype(np.float32)).to(_dev()).requires_grad_(True)
    th = torch.from_numpy(rs.standard_normal(B).astype(np.float32)).to(_dev())
    tl = torch.from_numpy(rs.standard_normal(B).astype(np.float32)).to(_dev())
    lh, ll, ph, pl = opt.forward_latent(z, (th, tl))
    (0.7 * lh + 1.3 * ll).backward()
    homo, lumo = _layers(opt)
    ref = po.heads_step(homo, lumo, z.detach().cpu().numpy().astype(np.float64), half, th.cpu().numpy().astype(np.float64),
                        tl.cpu().numpy().astype(np.float64), p=dropout, seed=(12345, 678), dloss=(0.7, 1.3))
    assert_close(ph.cpu().numpy(), ref["pred"][0], "homo pred")
    assert_close(pl.cpu().numpy(), ref["pred"][1], "lumo pred")
    assert abs(float(lh) - ref["loss"][0]) <= TOL * max(1.0, ref["loss"][0])
    assert abs(float(ll) - ref["loss"][1]) <= TOL * max(1.0, ref["loss"][1])
    assert_close(z.grad.cpu().numpy(), ref["dz"], "dz")
    for hi, head in enumerate((opt.homo_linear, opt.lumo_linear)):
        for i, lin in enumerate(head.linears()):
            assert_close(lin.weight.grad.cpu().numpy(), ref["grads"][hi][i][0], "dW %d.%d" % (hi, i))
            assert_close(lin.bias.grad.cpu().numpy(), ref["grads"][hi][i][1], "db %d.%d" % (hi, i))


def test_heads_eval_mode_ignores_dropout_and_one_row_is_0d():
    opt = _heads(12, [64, 64], 0.1)
    opt.eval()
    rs = np.random.RandomState(1)
    z = torch.from_numpy(rs.standard_normal((5, 24)).astype(np.float32)).to(_dev())
    t = torch.zeros(5, device=_dev())
    _, _, ph, pl = opt(z[:, :12], z[:, 12:], (t, t))
    homo, lumo = _layers(opt)
    ref = po.heads_step(homo, lumo, z.cpu().numpy().astype(np.float64), 12, np.zeros(5), np.zeros(5))
    assert_close(ph.cpu().numpy(), ref["pred"][0], "eval homo")
    assert_close(pl.cpu().numpy(), ref["pred"][1], "eval lumo")
    h1, l1 = opt.predict(z[0, :12], z[0, 12:])
    assert h1.dim() == 0 and l1.dim() == 0
    assert abs(float(h1) - ref["pred"][0][0]) <= TOL * max(1, abs(ref["pred"][0][0]))


@pytest.mark.parametrize("publish", [True, False])
def test_heads_gradients_add_into_existing_grad_and_are_bitwise_reproducible(publish):
    from ggpm_amd import functional as F_
    prev = F_.publish_gradients(publish)
    try:
        runs = []
        for _ in range(2):
            opt = _heads(12, [64, 64], 0.0, seed=5)
            start = {k: torch.full_like(p, 0.25) for k, p in opt.named_parameters()}
            for k, p in opt.named_parameters():
                p.grad = start[k].clone()
            rs = np.random.RandomState(7)
            z = torch.from_numpy(rs.standard_normal((20, 24)).astype(np.float32)).to(_dev()).requires_grad_(True)
            t = torch.from_numpy(rs.standard_normal(20).astype(np.float32)).to(_dev())
            lh, ll, _, _ = opt.forward_latent(z, (t, -t))
            (lh + ll).backward()
            fresh = _heads(12, [64, 64], 0.0, seed=5)
            zf = z.detach().clone().requires_grad_(True)
            a, b, _, _ = fresh.forward_latent(zf, (t, -t))
            (a + b).backward()
            for (k, p), (_, q) in zip(opt.named_parameters(), fresh.named_parameters()):
                assert torch.equal(p.grad, start[k] + q.grad), k
            torch.cuda.synchronize()
            runs.append([p.grad.clone() for p in opt.parameters()] + [z.grad.clone(), lh.detach().clone()])
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    finally:
        F_.publish_gradients(prev)


def test_heads_outside_the_envelope_raise_not_implemented():
    opt = _heads(12, [600], 0.0)
    z = torch.zeros(4, 24, device=_dev())
    with pytest.raises(NotImplementedError):
        opt.forward_latent(z, (torch.zeros(4, device=_dev()), torch.zeros(4, device=_dev())))


# ------------------------------------------------------------------------------------------ HierPropOptVAE
def _propopt_model(g):
    from ggpm_amd import synth
    from ggpm_amd.decoder import DecodeSchedule
    from ggpm_amd.property_vae import HierPropOptVAE
    from ggpm_amd.vocab import IndexPairVocab
    specs = g.specs()
    tensors = synth.tensorize(specs)
    model = HierPropOptVAE(g.args(IndexPairVocab(g.n_motif, g.n_attach))).to(_dev())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in g.state_dict().items()}, strict=False)
    assert not res.unexpected_keys
    assert all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.")) for k in res.missing_keys), res.missing_keys
    return model, tensors, DecodeSchedule.from_specs(specs, tensors)


def _step(g, model, tensors, sch, **kw):
    return model(None, None, tensors, [None] * g.B, g.z["t_homo"].tolist(), g.z["t_lumo"].tolist(), beta=0.1,
                 perturb_z=False, schedule=sch, **kw)


@pytest.mark.parametrize("name", pf.names("propopt"))
@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hierpropoptvae_step_matches_reference_golden(name, lazy, monkeypatch):
    """Loss, every metric, every gradient of the reference's HierPropOptVAE step.  None gradients: R_var's stays None
    (perturb_z=False: no KL term in the loss).  The reference leaves the tree encoder's W_o None as well -- it does not
    take part in the tree level --, where this package's fused encoder node has always returned a zero gradient; that
    parameter must then be None or exactly zero."""
    monkeypatch.setenv("GGPM_LAZY_METRICS", lazy)
    g = pf.PropOptGolden(name)
    model, tensors, sch = _propopt_model(g)
    loss, metrics, clipped = _step(g, model, tensors, sch)
    loss.backward()
    assert not bool(clipped)
    want = float(g.z["loss"])
    assert abs(float(loss.detach().reshape(-1)[0]) - want) <= TOL * abs(want)
    assert list(metrics.keys()) == list(g.metrics().keys())
    for k, v in g.metrics().items():
        assert abs(metrics[k] - v) <= TOL * max(1.0, abs(v)) + (1e-6 if k in ("Word", "I-Word", "Topo", "Assm") else 0), k
    ref_none = set(str(k) for k in g.z["none_grads"])
    for k, p in model.named_parameters():
        if p.grad is None:
            assert k in ref_none, "%s: no gradient here, one in the reference" % k
            continue
        if k in ref_none:
            assert k.startswith("encoder.tree_encoder.W_o") and not bool(p.grad.ne(0).any()), k
            continue
        want = g.z["grad/" + k].astype(np.float64)
        got = p.grad.detach().cpu().numpy().astype(np.float64)
        scale = np.abs(want).max()
        if scale < 1e-7 or k.endswith("W_assm.bias"):
            assert np.abs(got).max() < 1e-4, k
            continue
        assert np.abs(got - want).max() / scale <= TOL, "%s grad: rel err %.3e" % (k, np.abs(got - want).max() / scale)
    assert model.R_var.weight.grad is None and model.R_var.bias.grad is None


def test_fine_tune_loop_shape_save_load_and_pretrained_checkpoint(tmp_path):
    """vae_fine_tune.py's loop on the model: the 3-tuple, zero_grad -> backward -> clip_grad_norm_ -> Adam, a
    model.eval() + no_grad validation forward, save / load, and a HierPropertyVAE checkpoint copied in through the
    encoder / decoder sub-dicts (ggpm/nnutils.py copy_model)."""
    from ggpm_amd.property_vae import HierPropOptVAE, HierPropertyVAE
    from ggpm_amd.vocab import IndexPairVocab
    g = pf.PropOptGolden("propopt_lstm_s51")
    model, tensors, sch = _propopt_model(g)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        model.zero_grad()
        model.train()
        loss, metrics, clipped = _step(g, model, tensors, sch)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 20.0)
        optimizer.step()
        losses.append(float(metrics["Loss"]))
        assert not bool(clipped)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    model.eval()
    with torch.no_grad():
        vloss, vmetrics, _ = _step(g, model, tensors, sch)
    assert np.isfinite(float(vloss)) and set(vmetrics.keys()) == set(g.metrics().keys())
    path = tmp_path / "model.0"
    torch.save(model.state_dict(), path)
    again, _, _ = _propopt_model(g)
    again.load_state_dict(torch.load(path))
    again.eval()
    with torch.no_grad():
        l2, _, _ = _step(g, again, tensors, sch)
    assert torch.equal(vloss, l2)
    pre = HierPropertyVAE(g.args(IndexPairVocab(g.n_motif, g.n_attach))).to(_dev())
    fine = HierPropOptVAE(g.args(IndexPairVocab(g.n_motif, g.n_attach))).to(_dev())
    fine.encoder.load_state_dict(pre.encoder.state_dict())
    fine.decoder.load_state_dict(pre.decoder.state_dict())
    for k, v in pre.encoder.state_dict().items():
        assert torch.equal(fine.encoder.state_dict()[k], v)


def test_clip_negative_loss_replaces_the_loss_on_the_device_and_keeps_the_global_rng():
    """loss_scaling with the heads predicting their targets exactly (HOMO / LUMO MSE 0) and log-variances of -500 makes
    the total negative: the flag is true, the loss is a draw of N(0.5, 0.5) from the model's own generator, every
    gradient is zero, and torch's global CUDA generator has not moved."""
    g = pf.PropOptGolden("propopt_gru_s52")
    model, tensors, sch = _propopt_model(g)
    with torch.no_grad():
        for head, t in ((model.property_optim.homo_linear, 0.25), (model.property_optim.lumo_linear, -0.5)):
            last = head.linears()[-1]
            last.weight.zero_()
            last.bias.fill_(t)
        model.loss_weigh.homo_log_var.fill_(-500.0)
        model.loss_weigh.lumo_log_var.fill_(-500.0)
    state = torch.cuda.get_rng_state()
    loss, metrics, clipped = model(None, None, tensors, [None] * g.B, [0.25] * g.B, [-0.5] * g.B, beta=0.1,
                                   perturb_z=False, schedule=sch)
    loss.sum().backward()
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert bool(clipped)
    assert metrics["HOMO_MSE"] == -500.0 and metrics["LUMO_MSE"] == -500.0
    assert float(loss.reshape(-1)[0]) != float(metrics["Recs_Loss"]) - 1000.0
    for k, p in model.named_parameters():
        assert p.grad is None or not bool(p.grad.ne(0).any()), k


# ------------------------------------------------------------------------------------------ latent search
class _Args:
    def __init__(self, mode, steps, patience, thr, delta, lr, max_steps=10000):
        self.optimize_type, self.property_optim_step, self.patience = mode, steps, patience
        self.patience_threshold, self.property_delta, self.latent_lr, self.max_steps = thr, delta, lr, max_steps


class _Holder(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.property_optim = opt
        self.latent_size = opt.input_size


def _search_model(z):
    from ggpm_amd.property import PropertyOptimizer
    lh = [int(v) for v in z["linear_hidden"]]
    half = int(z["latent"]) // 2
    opt = PropertyOptimizer(half, lh[0] if len(lh) == 1 else lh, 0.1)
    opt.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    return _Holder(opt.to(_dev()).eval()), half


@pytest.mark.parametrize("name", pf.names("propsearch"))
def test_latent_search_matches_the_reference(name):
    """Step counts exactly; final latents and predictions within max(1e-4, 4 x the reference fp32 run's own distance
    to its fp64 run) per element -- the calibrated bound of this project's oracle tests.  Parameter .grads untouched."""
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    z = pf.load(name)
    model, half = _search_model(z)
    patience, thr, delta, lr = [float(v) for v in z["params"]]
    mode = str(z["mode"])
    marker = [torch.full_like(p, 3.0) for p in model.parameters()]
    for p, m in zip(model.parameters(), marker):
        p.grad = m.clone()
    search = HierPropertyVAEOptimizer(model, _Args(mode, int(z["steps"]), patience, thr, delta, lr))
    zz = torch.from_numpy(z["z"]).to(_dev())
    fn = search._get_optimize_func()
    out = fn(zz[:, :half], zz[:, half:], torch.from_numpy(z["t_homo"]), torch.from_numpy(z["t_lumo"]))
    assert (search.steps_taken.cpu().numpy() == z["steps_ref"]).all(), (search.steps_taken.tolist(), z["steps_ref"])
    assert (search.status.cpu().numpy() == 0).all()
    ref, ref64 = z["z_ref"].astype(np.float64), z["z_ref64"]
    bound = np.maximum(1e-4, 4 * np.abs(ref - ref64))
    err = np.abs(out.cpu().numpy() - ref)
    assert (err <= bound).all(), "latent: worst excess %.3e" % (err - bound).max()
    pred = torch.stack(search.predictions).cpu().numpy()
    pref, pref64 = z["pred_ref"].astype(np.float64), z["pred_ref64"]
    pbound = np.maximum(1e-4, 4 * np.abs(pref - pref64))
    assert (np.abs(pred - pref) <= pbound).all()
    for p, m in zip(model.parameters(), marker):
        assert torch.equal(p.grad, m)


@pytest.mark.parametrize("B,steps", [(1, 5), (20, 50), (256, 200)])
def test_latent_search_is_one_kernel_launch(B, steps):
    from torch.profiler import profile, ProfilerActivity
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    model = _Holder(_heads(12, [64, 64], 0.1).eval())
    search = HierPropertyVAEOptimizer(model, _Args("fixed", steps, 5, 0.1, 0.1, 1.0))
    rs = np.random.RandomState(B)
    z = torch.from_numpy(rs.standard_normal((B, 24)).astype(np.float32)).to(_dev())
    t = torch.from_numpy(rs.standard_normal(B).astype(np.float32)).to(_dev())
    search.hard_optimize(z[:, :12], z[:, 12:], t, -t)          # warm-up
    torch.cuda.synchronize()
    zc = torch.cat([z[:, :12], z[:, 12:]], -1)             # (the concatenation of the two halves is plumbing: outside)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        search._search("fixed", zc[:, :12], zc[:, 12:], t, -t)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    searches = [n for n in names if "prop_search_k" in n]
    assert len(searches) == 1, names
    assert (search.steps_taken == steps).all()


def test_latent_search_raises_for_heads_in_training_mode_with_dropout():
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    model = _Holder(_heads(12, [64, 64], 0.1).train())
    search = HierPropertyVAEOptimizer(model, _Args("soft", 5, 5, 0.1, 0.1, 1.0))
    z = torch.zeros(2, 24, device=_dev())
    with pytest.raises(RuntimeError, match="eval"):
        search.soft_optimize(z[:, :12], z[:, 12:], torch.zeros(2), torch.zeros(2))


def test_latent_search_caps_a_zero_loss_patience_search():
    """The heads predict their targets exactly: loss 0, |0 - 0| / 0 = NaN, the patience resets every body -- the
    reference never returns.  Here every molecule ends capped after max_steps bodies, with a warning, in bounded time."""
    from ggpm_amd.property_control import HierPropertyVAEOptimizer
    opt = _heads(12, [64, 64], 0.0)
    with torch.no_grad():
        for head, t in ((opt.homo_linear, 0.25), (opt.lumo_linear, -0.5)):
            head.linears()[-1].weight.zero_()
            head.linears()[-1].bias.fill_(t)
    search = HierPropertyVAEOptimizer(_Holder(opt.eval()), _Args("patience", 20, 5, 0.1, 0.1, 1.0, max_steps=1000))
    z = torch.randn(8, 24, device=_dev())
    t0 = time.perf_counter()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = search.patience_optimize(z[:, :12], z[:, 12:], torch.full((8,), 0.25), torch.full((8,), -0.5))
        torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 30
    assert any("max_steps=1000" in str(x.message) for x in w)
    assert (search.status == 1).all() and (search.steps_taken == 1000).all()
    assert torch.equal(out, z)
