"""GPU: a backward pass ADDS into whatever ``.grad`` already holds, on every path by which this package writes ``.grad``
itself -- the deferred weight-gradient flush (end of pass and early, on the second stream), the second-stream writers
(``functional._accumulate_grad``), the deferred sums of the sparse message functions, the atom-level decode's end-of-pass
callback and the encoder's gradient sink into ``parallel.FlatGradSync``'s flat buffer -- and the flat buffer's per-parameter
slots live no longer than the sync that owns them.

Every backward under test runs with the caching allocator's free blocks filled with NaN (``poison_free_blocks``), so that
a gradient read before it is written shows as NaN rather than as plausible numbers."""
import copy
import gc

import numpy as np
import pytest
import torch
import torch.nn as nn

from golden_utils import VaeGolden, vae_model

pytestmark = pytest.mark.gpu

TOL = 1e-4          # BASELINE.json: the kernels against the reference's vectors
MECH_TOL = 1e-5     # small graphs against their fp64 reference, per tensor, of the reference's max|.|
SUM_TOL = 1e-6      # an accumulated gradient against the sum of single-pass gradients: fp32 addition order only


def _dev():
    return torch.device("cuda:0")


def poison_free_blocks(params, dev=None):
    """Best effort: allocate ``torch.full_like(p, nan)`` for every parameter shape and free it again, on the main stream and
    on the package's second stream (the caching allocator hands a freed block out again only to the stream that freed it).
    A gradient buffer that is read before it is written then tends to show NaN instead of stale, plausible numbers.  Nothing
    guarantees the next allocation reuses these blocks: the value comparisons of the tests are what decides."""
    from ggpm_amd import functional as F_
    dev = dev or _dev()
    for s in (torch.cuda.current_stream(dev), F_._side_stream(dev)):
        with torch.cuda.stream(s):
            junk = [torch.full_like(p, float("nan")) for p in params]
            del junk
    torch.cuda.synchronize(dev)


def _backward(fwd, params):
    loss = fwd()
    poison_free_blocks(params)
    loss.backward()
    torch.cuda.synchronize()


def _close(got, want, scale, tol, what):
    got = got.detach().double().cpu()
    err = float((got - want).abs().max())
    assert err == err and err <= tol * scale, "%s: max err %.3e of scale %.3e" % (what, err, scale)


def _check_start_states(module, fwd, want, tol=MECH_TOL):
    """``fwd()`` -> a loss over ``module``'s parameters; ``want`` {name: fp64 CPU gradient} of one backward of it.  From
    ``.grad`` None, from a seeded non-zero G0, two backwards without zeroing, zero_grad(set_to_none=False) + one backward."""
    named = [(k, p) for k, p in module.named_parameters() if k in want]
    params = [p for _, p in named]
    scale = {k: max(float(want[k].abs().max()), 1e-30) for k, _ in named}
    gen = torch.Generator().manual_seed(11)
    G0 = {k: (torch.randn(p.shape, generator=gen, dtype=torch.float64) * scale[k]).float() for k, p in named}

    module.zero_grad(set_to_none=True)
    _backward(fwd, params)
    for k, p in named:
        _close(p.grad, want[k], scale[k], tol, "from None: " + k)

    for k, p in named:
        p.grad = G0[k].to(p.device)
    _backward(fwd, params)
    for k, p in named:
        _close(p.grad, G0[k].double() + want[k], scale[k], tol, "from G0: " + k)

    module.zero_grad(set_to_none=True)
    _backward(fwd, params)
    _backward(fwd, params)
    for k, p in named:
        _close(p.grad, 2 * want[k], 2 * scale[k], tol, "two backwards: " + k)

    module.zero_grad(set_to_none=False)
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in params)
    _backward(fwd, params)
    for k, p in named:
        _close(p.grad, want[k], scale[k], tol, "zero_grad(set_to_none=False): " + k)


def _fp64_grads(module, loss_fn):
    """Gradients of ``loss_fn(fp64 CPU copy of module)`` -> {name: tensor}."""
    ref = copy.deepcopy(module).double().cpu()
    ref.zero_grad(set_to_none=True)
    loss_fn(ref).backward()
    return {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------------------------------ the deferred queue
def test_one_weight_visited_with_two_k_splits_in_one_pass():
    """One Linear used under K split [24] and under [12, 12] in the same pass: two queue entries for one parameter, whose
    contractions must BOTH land in .grad (the second is added to the first)."""
    from ggpm_amd import functional as F_
    dev = _dev()
    torch.manual_seed(0)
    lin = nn.Linear(24, 32).to(dev)
    x1 = torch.randn(9, 24)
    x2 = torch.randn(13, 24)
    c1, c2 = torch.randn(9, 32), torch.randn(13, 32)
    g = [t.to(dev) for t in (x1, x2, c1, c2)]
    x2a, x2b = g[1][:, :12].contiguous(), g[1][:, 12:].contiguous()

    def fwd():
        y1 = F_.linear([g[0]], [24], lin.weight, lin.bias)
        y2 = F_.linear([x2a, x2b], [12, 12], lin.weight, lin.bias)
        return (y1[:, :32] * g[2]).sum() + (y2[:, :32] * g[3]).sum()

    want = _fp64_grads(lin, lambda m: (m(x1.double()) * c1.double()).sum() + (m(x2.double()) * c2.double()).sum())
    _check_start_states(lin, fwd, want)


class _FlushEarly(torch.autograd.Function):
    """Identity whose backward runs the deferred queue's early flush (as the atom-level decode's node does)."""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, dx):
        from ggpm_amd import functional as F_
        F_.flush_deferred_early()
        _FlushEarly.seen.append(F_._DEFERRED.early is not None)
        return dx


def test_one_weight_visited_on_both_sides_of_the_early_flush(monkeypatch):
    """One square Linear used before and after a node whose backward flushes the queue early: the later visit's
    contraction is published by the early flush (second stream, handed over at the end of the pass), the earlier one's
    by the end-of-pass flush, into the same .grad."""
    from ggpm_amd import _dev as dev_settings, functional as F_
    monkeypatch.setenv("GGPM_SIDE_STREAM", "1")
    monkeypatch.setattr(dev_settings, "DEFER_EARLY", True)
    dev = _dev()
    torch.manual_seed(1)
    lin = nn.Linear(16, 16).to(dev)
    x, c = torch.randn(11, 16), torch.randn(11, 16)
    xd, cd = x.to(dev), c.to(dev)

    def fwd():
        h = F_.linear([xd], [16], lin.weight, lin.bias)
        h2 = _FlushEarly.apply(h[:, :16].contiguous())
        y = F_.linear([h2], [16], lin.weight, lin.bias)
        return (y[:, :16] * cd).sum()

    want = _fp64_grads(lin, lambda m: (m(m(x.double())) * c.double()).sum())
    _FlushEarly.seen.clear()
    _check_start_states(lin, fwd, want)
    assert _FlushEarly.seen and all(_FlushEarly.seen), "the early flush did not run"


class _Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(11, 24)
        self.lin1 = nn.Linear(24, 32)
        self.lin2 = nn.Linear(32, 8)


def _small_case(dev):
    """Embedding gather -> Linear + ReLU -> Linear, as F_ ops on the GPU and as plain fp64 ops on the CPU."""
    from ggpm_amd import functional as F_
    torch.manual_seed(2)
    m = _Small().to(dev)
    idx = torch.tensor([1, 5, 5, 7, 0, 10, 3, 3, 3], dtype=torch.int64)
    c = torch.randn(9, 8)
    idx_d = idx.to(dev).int()
    idx_csr = F_.csr_from_index(idx_d, ncols=11)
    cd = c.to(dev)

    def fwd_of(mod):
        def fwd():
            x = F_.gather_rows(mod.emb.weight, idx_d, idx_csr, 24, 24)
            h = F_.linear([x], [24], mod.lin1.weight, mod.lin1.bias, act=F_.ACT_RELU)
            y = F_.linear([h[:, :32].contiguous()], [32], mod.lin2.weight, mod.lin2.bias)
            return (y[:, :8] * cd).sum() + h[:, :32].sum()
        return fwd

    def ref(r):
        h = torch.relu(r.lin1(r.emb(idx)))
        return (r.lin2(h) * c.double()).sum() + h.sum()

    return m, fwd_of, _fp64_grads(m, ref)


@pytest.mark.parametrize("defer,side", [("1", "1"), ("0", "1"), ("0", "0")],
                         ids=["deferred", "second_stream", "main_stream"])
def test_linear_and_embedding_gradients_add_into_existing_grad(defer, side, monkeypatch):
    """_Linear / _GatherRows on each of their gradient paths: deferred to the end-of-pass flush (default), formed on the
    second stream and added by _accumulate_grad (GGPM_DEFER_WGRADS=0), returned through autograd (both switches off)."""
    monkeypatch.setenv("GGPM_DEFER_WGRADS", defer)
    monkeypatch.setenv("GGPM_SIDE_STREAM", side)
    m, fwd_of, want = _small_case(_dev())
    _check_start_states(m, fwd_of(m), want)


def _level_case(rnn, dev, E=40, I=13, H=24, depth=3, K=4):
    from ggpm_amd import rnn as R
    from ggpm_amd.params import rnn_param_shapes, seeded_state_dict
    from oracle import ref_encoder as ref
    rs = np.random.RandomState(E + I + H + depth)
    bgraph = np.zeros((E + 1, K + 1), dtype=np.int64)
    for e in range(1, E + 1):
        k = rs.randint(0, K + 1)
        bgraph[e, :k] = rs.choice(np.arange(1, E + 1), size=k, replace=False)
    x = rs.standard_normal((E + 1, I)).astype(np.float32)
    w = rs.standard_normal((E + 1, H)).astype(np.float32)
    sd = seeded_state_dict(rnn_param_shapes(rnn, I, H), seed=E + H)
    mod = (R.GRU if rnn == "GRU" else R.LSTM)(I, H, depth).to(dev)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    xd, bd, wd = (torch.from_numpy(a).to(dev) for a in (x, bgraph, w))

    def fwd():
        out = mod(xd, bd)
        return ((out if rnn == "GRU" else out[0]) * wd).sum()

    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    href = ref.rnn_forward(p, "", rnn, torch.from_numpy(x).double(), torch.from_numpy(bgraph), depth)
    (href * torch.from_numpy(w).double()).sum().backward()
    return mod, fwd, {k: v.grad.detach().clone() for k, v in p.items()}


@pytest.mark.parametrize("side", ["1", "0"])
@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_level_function_gradients_add_into_existing_grad(rnn, side, monkeypatch):
    """F_.gru_level / F_.lstm_level (rnn.GRU / rnn.LSTM forward) against the fp64 oracle: with the second stream their
    parameter gradients are added by _accumulate_grad there, without it they return through autograd."""
    monkeypatch.setenv("GGPM_SIDE_STREAM", side)
    mod, fwd, want = _level_case(rnn, _dev())
    _check_start_states(mod, fwd, want)


def _sparse_case(rnn, dev, E1=120, I=28, H=32, depth=2, ms=40):
    from golden_utils import sparse_inputs
    from ggpm_amd import rnn as R
    from ggpm_amd.params import rnn_param_shapes, seeded_state_dict
    from oracle import ref_encoder as ref
    h, c, submess, x, bg, coef = sparse_inputs(E1, I, H, ms, 4, E1 + H + depth)
    sd = seeded_state_dict(rnn_param_shapes(rnn, I, H), 3)
    mod = (R.GRU if rnn == "GRU" else R.LSTM)(I, H, depth).to(dev)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hd, cd_ = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (h, c))
    xd = torch.from_numpy(x).to(dev)
    sm, bgt, cf = (torch.from_numpy(a).to(dev) for a in (submess, bg, coef))

    def fwd():
        if rnn == "GRU":
            return (cf[0] * mod.sparse_forward(hd, xd, sm, bgt)).sum()
        ho, co = mod.sparse_forward((hd, cd_), xd, sm, bgt)
        return (cf[0] * ho).sum() + (cf[1] * co).sum()

    p = {"rnn." + k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    hr, cr, xr = (torch.from_numpy(a).double() for a in (h, c, x))
    cf64 = torch.from_numpy(coef).double()
    if rnn == "GRU":
        loss = (cf64[0] * ref.gru_sparse_forward(p, "rnn.", hr, xr, torch.from_numpy(submess), torch.from_numpy(bg),
                                                 depth)).sum()
    else:
        ro, rc = ref.lstm_sparse_forward(p, "rnn.", hr, cr, xr, torch.from_numpy(submess), torch.from_numpy(bg), depth)
        loss = (cf64[0] * ro).sum() + (cf64[1] * rc).sum()
    loss.backward()
    return mod, fwd, {k[4:]: v.grad.detach().clone() for k, v in p.items()}


@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_sparse_function_gradients_add_into_existing_grad(rnn):
    """F_.gru_sparse / F_.lstm_sparse (the incremental encoder's message functions) against the fp64 oracle: their
    parameter gradients go through the deferred sums (_defer_sum) of the end-of-pass flush."""
    mod, fwd, want = _sparse_case(rnn, _dev())
    _check_start_states(mod, fwd, want)


# ------------------------------------------------------------------------------------------ the full VAE step
def _set_form(monkeypatch, mode="batched", side="1", defer_early=True, defer_wgrads="1"):
    """The forms of the device loop (ggpm_amd/_dev.py), as test_gpu_parity.test_vae_step_matches_reference_golden sets them."""
    from ggpm_amd import _dev as dev_settings
    monkeypatch.setattr(dev_settings, "DECODER_BATCHED", mode != "stepwise")
    monkeypatch.setattr(dev_settings, "ATOM_DECODE", mode.startswith("batched"))
    monkeypatch.setattr(dev_settings, "ATOM_AHEAD", mode == "batched")
    monkeypatch.setattr(dev_settings, "DEFER_EARLY", defer_early)
    monkeypatch.setenv("GGPM_SIDE_STREAM", side)
    monkeypatch.setenv("GGPM_DEFER_WGRADS", defer_wgrads)


class _Vae:
    def __init__(self, name):
        self.g, self.model, self.tensors, self.sch = vae_model(name, _dev())
        self.named = list(self.model.named_parameters())       # tied parameters once
        self.params = [p for _, p in self.named]

    def loss(self):
        g = self.g
        loss, _ = self.model(None, None, self.tensors, [None] * g.B, None, None, beta=g.beta, perturb_z=False,
                             schedule=self.sch)
        return loss

    def backward(self, retain=False):
        loss = self.loss()
        poison_free_blocks(self.params)
        loss.backward(retain_graph=retain)
        torch.cuda.synchronize()
        return loss

    def grads(self):
        return {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in self.named}

    def first(self):
        """g1: the same form once from .grad = None, checked against the reference's vectors."""
        self.model.zero_grad(set_to_none=True)
        self.backward()
        g1 = self.grads()
        for k, v in g1.items():
            self.g.check_grad(k, v.cpu().numpy(), rel=TOL)
        return g1


def _analytic_zero(g: VaeGolden, k):
    """VaeGolden.check_grad's rounding-noise-only gradients (their value is not a multiple of anything)."""
    if "grad/" + k in g.z.files:
        return float(np.abs(g.z["grad/" + k]).max()) < 1e-7 or k.endswith("W_assm.bias")
    return False


def _sum_close(g: VaeGolden, k, got, want, what):
    got = got.detach().double()
    want = want.detach().double()
    if _analytic_zero(g, k):
        assert float((got - want).abs().max()) < 1e-4, "%s %s" % (what, k)
        return
    err = float(torch.linalg.vector_norm(got - want))
    ref = float(torch.linalg.vector_norm(want))
    assert err == err and err <= SUM_TOL * max(ref, 1e-30), "%s %s: |d| %.3e of |want| %.3e" % (what, k, err, ref)


def _g0(g1, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(v.shape, generator=gen, dtype=torch.float64) * max(float(v.abs().max()), 1e-12)).float()
            .to(v.device) for k, v in g1.items()}


def _check_from_g0(v: _Vae, g1):
    G0 = _g0(g1, 5)
    for k, p in v.named:
        p.grad = G0[k].clone()
    v.backward()
    for k, p in v.named:
        v.g.check_grad(k, (p.grad - G0[k]).cpu().numpy(), rel=TOL)
        _sum_close(v.g, k, p.grad, G0[k] + g1[k], "G0 start")


def _vae_names():
    from golden_utils import vae_case_names
    return vae_case_names()


@pytest.mark.parametrize("start", ["g0", "twice", "zero_grad_keep"])
@pytest.mark.parametrize("name", _vae_names())
def test_vae_step_adds_into_existing_grad(name, start, monkeypatch):
    """The default form of the VAE step (every writer of .grad: deferred flush early and at the end, second stream, atom-
    level callback, encoder driver) from three start states: a seeded G0, two backwards without zeroing, and
    zero_grad(set_to_none=False) then one backward."""
    _set_form(monkeypatch)
    v = _Vae(name)
    g1 = v.first()
    if start == "g0":
        _check_from_g0(v, g1)
        return
    if start == "twice":
        v.model.zero_grad(set_to_none=True)
        v.backward()
        v.backward()
        for k, p in v.named:
            v.g.check_grad(k, (p.grad / 2).cpu().numpy(), rel=TOL)
            _sum_close(v.g, k, p.grad, 2 * g1[k], "two backwards")
        return
    v.model.zero_grad(set_to_none=False)
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in v.params)
    v.backward()
    for k, p in v.named:
        _sum_close(v.g, k, p.grad if p.grad is not None else torch.zeros_like(p), g1[k], "zero_grad(set_to_none=False)")


def _form_cases():
    out = []
    for name in ("vae_gru_s40", "vae_lstm_s41"):
        for mode in ("batched_inline", "levels", "stepwise"):
            for side in ("1", "0"):
                out.append(pytest.param(name, mode, side, True, "1", id="%s-%s-side%s" % (name, mode, side)))
        out.append(pytest.param(name, "batched", "1", False, "1", id="%s-no_early_flush" % name))
        out.append(pytest.param(name, "batched", "1", True, "0", id="%s-no_deferral" % name))
    return out


@pytest.mark.parametrize("name,mode,side,early,defer", _form_cases())
def test_vae_step_forms_add_into_existing_grad(name, mode, side, early, defer, monkeypatch):
    """The other forms of the device loop, with and without the second stream, the default form without the early flush and
    without deferral: each from a seeded G0."""
    _set_form(monkeypatch, mode, side, early, defer)
    v = _Vae(name)
    _check_from_g0(v, v.first())


@pytest.mark.parametrize("name", ["vae_gru_s42", "vae_lstm_s43"])
def test_bench_form_accumulates_two_backwards_in_the_flat_buffer(name, monkeypatch):
    """bench.py's VAE row: FlatGradSync(keep_flat=True) with the encoder's gradient sink and FlatAdam.  Two backwards, then
    all_reduce(): the second encoder backward takes the sink's accumulate branch, the decoder's second contributions are
    added into the slots the first ones were formed in."""
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    _set_form(monkeypatch)
    v = _Vae(name)
    sync = FlatGradSync(v.model.parameters(), encoder=v.model.encoder, keep_flat=True)
    FlatAdam(sync, lr=1e-3)
    sync.zero_grad()
    v.backward()
    sync.all_reduce()
    torch.cuda.synchronize()
    g1 = v.grads()
    for k, t in g1.items():
        v.g.check_grad(k, t.cpu().numpy(), rel=TOL)
    sync.zero_grad()
    v.backward()
    v.backward()
    sync.all_reduce()
    torch.cuda.synchronize()
    lo, hi = sync.flat.data_ptr(), sync.flat.data_ptr() + sync.flat.numel() * 4
    for k, p in v.named:
        assert lo <= p.grad.data_ptr() < hi, k
        _sum_close(v.g, k, p.grad, 2 * g1[k], "two backwards into the flat buffer")


@pytest.mark.parametrize("name", ["vae_gru_s40", "vae_lstm_s41"])
def test_retained_graph_second_backward_is_exact_or_refused(name, monkeypatch):
    """loss.backward(retain_graph=True) twice: either 2 * g1, or a RuntimeError that says a retained graph is not
    supported -- never a TypeError / AttributeError from a released node, never a silently different gradient."""
    _set_form(monkeypatch)
    v = _Vae(name)
    g1 = v.first()
    v.model.zero_grad(set_to_none=True)
    loss = v.loss()
    poison_free_blocks(v.params)
    loss.backward(retain_graph=True)
    try:
        loss.backward(retain_graph=True)
    except RuntimeError as e:
        assert "retain" in str(e) and "not supported" in str(e), str(e)
        torch.cuda.synchronize()
        # a refused second pass leaves nothing queued behind: the next step is whole again
        v.model.zero_grad(set_to_none=True)
        v.backward()
        for k, p in v.named:
            _sum_close(v.g, k, p.grad, g1[k], "the step after a refused second backward")
        return
    torch.cuda.synchronize()
    for k, p in v.named:
        _sum_close(v.g, k, p.grad, 2 * g1[k], "retained graph, two backwards")


# ------------------------------------------------------------------------------------------ flat-buffer slot lifetime
def _in(t, flat):
    lo = flat.data_ptr()
    return lo <= t.data_ptr() < lo + flat.numel() * flat.element_size()


def _deferred_params(m):
    return [m.emb.weight, m.lin1.weight, m.lin1.bias, m.lin2.weight, m.lin2.bias]


def test_gradients_do_not_land_in_a_discarded_sync(monkeypatch):
    from ggpm_amd.parallel import FlatGradSync
    monkeypatch.setenv("GGPM_DEFER_WGRADS", "1")
    m, fwd_of, want = _small_case(_dev())
    fwd = fwd_of(m)
    params = _deferred_params(m)
    a = FlatGradSync(m.parameters(), keep_flat=True)
    a.zero_grad()
    _backward(fwd, params)
    old_flat = a.flat
    assert all(_in(p.grad, old_flat) for p in params)      # formed in place while the sync lives
    kept = [p.grad for p in params]
    snap = [t.clone() for t in kept]
    del a
    gc.collect()
    m.zero_grad(set_to_none=True)
    _backward(fwd, params)
    for k, p in zip(("emb.weight", "lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"), params):
        assert not _in(p.grad, old_flat), k
        _close(p.grad, want[k], max(float(want[k].abs().max()), 1e-30), MECH_TOL, k)
    for t, s in zip(kept, snap):
        assert torch.equal(t, s)


def test_a_later_sync_takes_over_the_slots(monkeypatch):
    from ggpm_amd.parallel import FlatGradSync
    monkeypatch.setenv("GGPM_DEFER_WGRADS", "1")
    m, fwd_of, _ = _small_case(_dev())
    fwd = fwd_of(m)
    params = _deferred_params(m)
    a = FlatGradSync(m.parameters(), keep_flat=True)
    b = FlatGradSync(m.parameters(), keep_flat=True)
    b.zero_grad()
    _backward(fwd, params)
    for p in params:
        assert not _in(p.grad, a.flat) and _in(p.grad, b.flat)
        assert any(p.grad.data_ptr() == v.data_ptr() for v in b.views)
    # an inactive sync (one rank, no keep_flat) replaces them with nothing, and leaves none of its own
    c = FlatGradSync(m.parameters())
    assert not c.active()
    m.zero_grad(set_to_none=True)
    _backward(fwd, params)
    for p in params:
        assert not _in(p.grad, a.flat) and not _in(p.grad, b.flat) and not _in(p.grad, c.flat)


def test_a_deep_copy_writes_into_no_flat_buffer(monkeypatch):
    from ggpm_amd.parallel import FlatGradSync
    monkeypatch.setenv("GGPM_DEFER_WGRADS", "1")
    m, fwd_of, want = _small_case(_dev())
    sync = FlatGradSync(m.parameters(), keep_flat=True)
    m2 = copy.deepcopy(m)
    snap = sync.flat.clone()
    fwd = fwd_of(m2)
    params2 = _deferred_params(m2)
    _backward(fwd, params2)
    storages = set()
    for k, p in zip(("emb.weight", "lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"), params2):
        assert not _in(p.grad, sync.flat), k
        _close(p.grad, want[k], max(float(want[k].abs().max()), 1e-30), MECH_TOL, k)
        storages.add(p.grad.untyped_storage().data_ptr())
    assert len(storages) == len(params2)                       # no shared (copied) flat buffer behind them either
    assert torch.equal(sync.flat, snap)
