"""CPU: host-side bookkeeping of ggpm_amd.functional / nnutils that needs no kernel -- the index-structure memo's
staleness guard, the hints make_cuda leaves on index tensors, and the deferred-gradient queue's behaviour around a
backward pass that raises."""
import contextlib

import pytest
import torch

from ggpm_amd import functional as F_
from ggpm_amd import nnutils


def test_index_memo_is_invalidated_by_an_in_place_refill():
    """A resident index tensor that is refilled with the next batch (``t.copy_(...)``) must not be served the CSR of its
    old contents: the memo is keyed by the tensor's in-place version counter."""
    t = torch.arange(12, dtype=torch.int64).view(4, 3)
    assert F_._memo_get(t, "_ggpm_csr", 5) is None
    F_._memo_put(t, "_ggpm_csr", 5, "old-structure")
    assert F_._memo_get(t, "_ggpm_csr", 5) == "old-structure"
    assert F_._memo_get(t, "_ggpm_csr", 6) is None            # other key (ncols)
    t.copy_(torch.zeros(4, 3, dtype=torch.int64))               # refill in place
    assert F_._memo_get(t, "_ggpm_csr", 5) is None
    F_._memo_put(t, "_ggpm_csr", 5, "new-structure")
    assert F_._memo_get(t, "_ggpm_csr", 5) == "new-structure"
    t[0, 0] = 3                                                  # any in-place write counts
    assert F_._memo_get(t, "_ggpm_csr", 5) is None


def test_tensor_hints_do_not_survive_an_in_place_refill():
    """``ggpm_chain`` (how many steps the tree-side levels need) and ``ggpm_roots`` describe the tensor's CONTENTS."""
    t = torch.zeros(6, 4, dtype=torch.int64)
    nnutils.attach_hint(t, "ggpm_chain", 7)
    assert nnutils.read_hint(t, "ggpm_chain", 0) == 7
    v = t.view_as(t)
    assert nnutils.read_hint(v, "ggpm_chain", 0) == 0           # a fresh view object carries no hint (bench.py relies on it)
    t.add_(1)
    assert nnutils.read_hint(t, "ggpm_chain", 0) == 0           # stale: the full depth loop runs
    nnutils.attach_hint(t, "ggpm_chain", 3)
    assert nnutils.read_hint(t, "ggpm_chain", 0) == 3


def test_tree_chain_length_is_bounded_by_the_motif_count():
    from ggpm_amd import synth
    specs = synth.random_batch(3, 4, motifs=(3, 6), n_motif_vocab=30, n_attach_vocab=90)
    tree, graph = synth.tensorize(specs)
    chain = nnutils.tree_chain_length(tree[3])          # (the host half of make_cuda; the upload needs the GPU)
    assert 1 <= chain <= 6


class _FakeStream:
    """Stands in for a HIP stream: remembers what it was created with and what it was told to wait for; ``log`` (shared)
    keeps the order of the waits among whatever else a test appends."""
    device = torch.device("cpu")
    log = []

    def __init__(self, name="main", device=None, priority=0):
        self.name, self.priority, self.waited = name, priority, []
        if device is not None:
            self.device = device

    def wait_stream(self, other):
        self.waited.append(other)
        _FakeStream.log.append(("wait", self, other))


class _Visit(torch.autograd.Function):
    """Stands in for a decoder op: its backward queues a deferred parameter gradient and may raise afterwards."""

    @staticmethod
    def forward(ctx, x, param, boom):
        ctx.param, ctx.boom = param, boom
        ctx.save_for_backward(x)
        return x * param.detach().sum()

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        F_._defer_sum(ctx.param, torch.full_like(ctx.param, float((g * x).sum())))
        if ctx.boom:
            raise RuntimeError("injected failure inside the backward pass")
        return g * ctx.param.detach().sum(), None, None


@pytest.fixture
def fake_streams(monkeypatch):
    main = _FakeStream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: main)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    del _FakeStream.log[:]
    F_._DEFERRED.reset()
    yield main
    F_._DEFERRED.reset()


def test_deferred_gradients_survive_a_failed_backward(fake_streams):
    """the autograd engine does not run queued callbacks when a backward raises.  The next pass must start
    from a clean queue, flush at its end, and publish exactly its own gradients."""
    p = torch.nn.Parameter(torch.ones(3))
    x = torch.arange(4.0, requires_grad=True)

    def step(boom):
        p.grad = None
        y = _Visit.apply(_Visit.apply(x, p, False), p, boom)      # two visits of the same parameter in one pass
        y.sum().backward()

    step(False)
    want = p.grad.clone()
    assert want.abs().sum() > 0 and not F_._DEFERRED.sum and F_._DEFERRED.task is None
    with pytest.raises(RuntimeError, match="injected"):
        step(True)
    assert F_._DEFERRED.sum, "the failed pass left its visit queued (the engine skipped the callback)"
    leftovers = F_._DEFERRED.task
    assert leftovers is not None
    step(False)                                                    # a normal step after the failure
    assert torch.equal(p.grad, want), (p.grad, want)               # not doubled by the failed pass's leftovers, not missing
    assert not F_._DEFERRED.sum and F_._DEFERRED.task is None
    step(False)
    assert torch.equal(p.grad, want)


def test_parameters_with_hooks_are_not_published_behind_autograd():
    """A parameter with a tensor hook / post-accumulate-grad hook (hook-based clippers, reducers) must get its gradient
    through AccumulateGrad so that the hooks fire.  Hooks on the AccumulateGrad NODE (stock DDP's reducer) cannot be seen
    from Python: for those the whole mechanism is switched off with ``publish_gradients(False)``."""
    p = torch.nn.Parameter(torch.ones(2))
    q = torch.nn.Parameter(torch.ones(2))
    assert F_.can_publish(p, q, None)
    h = q.register_hook(lambda g: g)
    assert not F_.can_publish(p, q)
    h.remove()
    assert F_.can_publish(p, q)
    h = p.register_post_accumulate_grad_hook(lambda t: None)
    assert not F_.can_publish(p)
    h.remove()
    frozen = torch.nn.Parameter(torch.ones(2), requires_grad=False)
    assert not F_.can_publish(frozen)
    assert not F_.can_publish(p * 2)                               # not a leaf
    # a hook on the accumulate node (what stock DDP registers) is invisible ...
    acc = p.expand_as(p).grad_fn.next_functions[0][0]
    h = acc.register_hook(lambda *a: None)
    assert F_.can_publish(p)
    # ... hence the process-wide switch
    assert F_.publish_gradients(False) is True
    try:
        assert not F_.can_publish(p) and not F_.can_publish(p, q, None)
    finally:
        assert F_.publish_gradients(True) is False
    assert F_.can_publish(p)
    h.remove()


def test_deferred_linear_is_keyed_by_its_column_split(fake_streams):
    """Two visits of one weight with different K splits must not be contracted with the first visit's split."""
    w = torch.nn.Parameter(torch.ones(2, 6))

    class _Q(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            F_._defer_linear(w, None, torch.ones(3, 2), [torch.ones(3, 6)], (6,))
            F_._defer_linear(w, None, torch.ones(3, 2), [torch.ones(3, 2), torch.ones(3, 4)], (2, 4))
            F_._defer_linear(w, None, torch.ones(5, 2), [torch.ones(5, 6)], (6,))
            keys = sorted(k[1] for k in F_._DEFERRED.linear)
            assert keys == [(2, 4), (6,)]
            assert sorted(len(v[3]) for v in F_._DEFERRED.linear.values()) == [1, 2]
            F_._DEFERRED.linear.clear()                           # (the flush would need the GPU GEMM)
            return g

    x = torch.ones(2, requires_grad=True)
    _Q.apply(x).sum().backward()


def test_publish_aside_forms_on_the_second_stream_and_joins_at_the_end_of_the_pass(fake_streams, monkeypatch):
    """functional.publish_aside: the second stream waits for the current one BEFORE the gradients are formed, every tensor
    they are formed from is marked for it, a parameter without a gradient gets the very tensor, one with a gradient is
    added to in place, and the current stream's re-join is queued for the end of the pass -- once, not run yet."""
    class Engine:
        callbacks = []

        def queue_callback(self, fn):
            self.callbacks.append(fn)

    class Read:
        def __init__(self):
            self.marks = []

        def record_stream(self, stream):
            self.marks.append(stream)

    main, side = fake_streams, _FakeStream("second")
    monkeypatch.setattr(torch.autograd.Variable, "_execution_engine", Engine())
    monkeypatch.setattr(F_, "_HELPER_STREAMS", {(0, "second"): side})
    reads = [Read(), Read(), Read()]
    fresh, kept = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    kept.grad = torch.ones(3)
    ptr = kept.grad.data_ptr()
    made = [torch.full((3,), 2.0), torch.full((3,), 5.0), None]

    def grads_fn():
        _FakeStream.log.append(("grads",))
        return made

    F_.publish_aside(torch.device("cuda", 0), reads, (fresh, kept, None), grads_fn)
    assert _FakeStream.log == [("wait", side, main), ("grads",)]
    assert all(r.marks == [side] for r in reads)
    assert fresh.grad is made[0]
    assert kept.grad.data_ptr() == ptr and torch.equal(kept.grad, torch.full((3,), 6.0))
    assert len(Engine.callbacks) == 1 and main.waited == []        # queued, not run
    Engine.callbacks[0]()
    assert main.waited == [side]


class _Step(torch.autograd.Function):
    """Identity whose backward calls ``fn`` (a node that queues a gradient, or flushes the queue early)."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _backward_through(*fns):
    """One backward pass whose nodes call ``fns`` in that order."""
    y = torch.ones(2, requires_grad=True)
    for fn in reversed(fns):
        y = _Step.apply(y, fn)
    y.sum().backward()


def test_early_flush_is_published_by_the_end_of_pass_flush(fake_streams):
    """A contribution queued before an early flush and one queued after it, for the same parameter (sums: no GEMM): the
    early result waits in ``pending`` with ``.grad`` untouched, the end-of-pass flush waits for the second stream once and
    adds both; ``written_on`` makes the end-of-pass flush wait the same way."""
    main, side, Q = fake_streams, _FakeStream("second"), F_._DEFERRED
    a, b, g0 = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([10.0, 20.0, 30.0]), torch.tensor([100.0, 200.0, 300.0])
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = g0.clone()
    ptr, seen = p.grad.data_ptr(), {}

    def flush_early():
        Q.flush(side=side)
        seen.update(grad=p.grad.clone(), ptr=p.grad.data_ptr(), pending=[(q, g.clone()) for q, g in Q.pending],
                    early=Q.early, log=list(_FakeStream.log))

    _backward_through(lambda: F_._defer_sum(p, a.clone()), flush_early, lambda: F_._defer_sum(p, b.clone()))
    assert torch.equal(seen["grad"], g0) and seen["ptr"] == ptr                     # untouched until the pass ends
    assert len(seen["pending"]) == 1 and seen["pending"][0][0] is p and torch.equal(seen["pending"][0][1], a)
    assert seen["early"] is side
    assert seen["log"] == [("wait", side, main)]                   # the early flush is ordered behind the queueing stream
    assert torch.equal(p.grad, g0 + a + b) and p.grad.data_ptr() == ptr
    assert Q.pending == [] and Q.early is None and Q.task is None
    assert main.waited == [side]                                   # exactly once

    del main.waited[:]
    p.grad = None
    _backward_through(lambda: (F_._defer_sum(p, a.clone()), Q.written_on(side)))
    assert main.waited == [side] and torch.equal(p.grad, a)
    assert Q.pending == [] and Q.early is None and Q.task is None


def test_helper_streams_come_from_one_table(monkeypatch):
    """functional.helper_stream: one stream per (device, kind), created on first request with that request's priority;
    writer_streams lists exactly the streams that exist."""
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None, priority=0: _FakeStream("made", device, priority))
    monkeypatch.setattr(F_, "_HELPER_STREAMS", {})
    dev = torch.device("cuda", 0)
    assert F_.writer_streams(dev) == []
    second = F_._side_stream(dev)
    assert F_.writer_streams(dev) == [second]
    atom = F_.helper_stream(dev, "atom", priority=-1)
    assert atom is not second and F_.writer_streams(dev) == [second, atom]
    assert F_._side_stream(dev) is second and F_.helper_stream(dev, "second") is second
    assert F_.helper_stream(dev, "atom") is atom and F_.helper_stream(dev, "atom", priority=-1) is atom
    assert (second.priority, atom.priority) == (0, -1) and atom.device == dev
    assert F_.writer_streams(torch.device("cuda", 1)) == []


@pytest.mark.parametrize("name", ["vae_lstm_s41", "vae_gru_s42"])
def test_state_dict_keys_are_the_references(name):
    """The parameter names of the reference's own HierPropertyVAE (recorded with its gradients in the fixtures) are
    exactly the drop-in's ``named_parameters``; ``state_dict`` adds only the two aliases the reference registers too
    (``decoder.rnn_cell``, ``decoder.E_assm``, ggpm/decoder.py:31-32)."""
    from golden_utils import VaeGolden
    from ggpm_amd.property_vae import HierPropertyVAE
    from ggpm_amd.vocab import IndexPairVocab
    g = VaeGolden(name)
    ref_names = {k.split("/", 1)[1] for k in g.z.files if k.startswith(("grad/", "gstat/"))}
    model = HierPropertyVAE(g.args(IndexPairVocab(g.n_motif, g.n_attach)))
    ours = {k for k, _ in model.named_parameters()}
    assert ours == ref_names, (sorted(ours - ref_names), sorted(ref_names - ours))
    extra = set(model.state_dict()) - ours
    assert extra and all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.")) or (g.tie and k.startswith("decoder.hmpn.E_"))
                         for k in extra), sorted(extra)


def test_published_gradients_are_not_stream_marked_by_default():
    """functional.hand_to: a gradient handed from a helper stream to the main stream gets no record_stream mark (on ROCm
    each mark is an event record on that stream when the tensor is released); _dev.RECORD_GRADS = True restores it"""
    from ggpm_amd import functional as F_

    class Probe:
        marks = 0

        def record_stream(self, stream):
            Probe.marks += 1

    from ggpm_amd import _dev
    F_.hand_to(Probe(), object())
    assert Probe.marks == (1 if _dev.RECORD_GRADS else 0)
    # the setting is read at call time: flipping it after import takes effect
    was, _dev.RECORD_GRADS = _dev.RECORD_GRADS, not _dev.RECORD_GRADS
    try:
        before = Probe.marks
        F_.hand_to(Probe(), object())
        assert Probe.marks - before == (1 if _dev.RECORD_GRADS else 0)
    finally:
        _dev.RECORD_GRADS = was



def test_index_structures_and_ctypes_marshalling_create_no_reference_cycles():
    """The host objects the step builds per call are freed by reference counting: the CSR remembered on an index
    tensor does not lead back to that tensor object, a transpose names its source weakly, array types are remembered."""
    import ctypes
    import gc
    import weakref
    import torch
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    assert _lib.array_type(ctypes.c_void_p, 3) is _lib.array_type(ctypes.c_void_p, 3)
    assert _lib.array_type(ctypes.c_int, 3) is not _lib.array_type(ctypes.c_int, 4)
    gc.collect()
    gc.disable()
    try:
        idx = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
        csr = F_.csr_from_index(idx, 3)
        assert F_.csr_from_index(idx, 3) is csr                      # remembered on the tensor ...
        assert csr.col is not idx and csr.col.data_ptr() == idx.data_ptr()      # ... through an alias, not the object itself
        t = F_.CSR(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 3, 4)
        t._back = weakref.ref(csr)                                   # (what _build_T sets on a transpose)
        assert t.T is csr
        probe = weakref.ref(csr)
        del csr, idx, t
        assert probe() is None, "the CSR of an index tensor is kept alive by a reference cycle"
        arr = _lib.array_type(ctypes.c_void_p, 2)(1, 2)
        assert ctypes.addressof(arr) and arr._objects is None        # (ctypes.cast(arr, c_void_p) would store arr in arr._objects)
    finally:
        gc.enable()


def test_bench_harness_term_equals_the_plain_sum_of_the_outputs():
    """bench.py drives a gradient into every encoder output with ``1e-3 * (hroot.sum() + hnode.sum() + hinter.sum() +
    hatom.sum())``; over outputs that are row ranges of one buffer it forms that term as ONE reduction and its gradient as ONE
    fill (bench._SumOutputs).  Same value, same gradients -- also when the outputs are not views of one buffer."""
    import torch
    import bench
    torch.manual_seed(0)

    class Four(torch.autograd.Function):         # four outputs that are row ranges of one buffer, like fused._HierEncoder
        @staticmethod
        def forward(ctx, x):
            out = x * 2.0
            return out.split([3, 5, 5, 11])

        @staticmethod
        def backward(ctx, *g):
            assert all(t.is_contiguous() for t in g)
            return torch.cat(g, dim=0) * 2.0

    for views in (True, False):
        x = torch.randn(24, 8, dtype=torch.float64, requires_grad=True)
        outs = Four.apply(x) if views else tuple(t * 2.0 for t in x.split([3, 5, 5, 11]))
        a = 1e-3 * bench._sum_outputs(*outs)
        ga, = torch.autograd.grad(a, x)
        x2 = x.detach().clone().requires_grad_(True)
        outs2 = tuple(t * 2.0 for t in x2.split([3, 5, 5, 11]))
        b = 1e-3 * (outs2[0].sum() + outs2[1].sum() + outs2[2].sum() + outs2[3].sum())
        gb, = torch.autograd.grad(b, x2)
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b)) and torch.equal(ga, gb), views
    ragged = (torch.ones(2, 3, requires_grad=True), torch.ones(2, 4, requires_grad=True))
    assert float(bench._sum_outputs(*ragged)) == 14.0


def test_bench_dump_outputs_are_float_bounded_and_reproducible(tmp_path):
    """``bench.py --dump-outputs DIR``: one DIR/<name>.npy per array, float32 (float64 kept), at most 64 MB in all; past the
    budget the large arrays are cut to a seeded sample, the same positions on every run, and small ones stay whole."""
    import glob
    import os
    import numpy as np
    import pytest
    import bench
    rng = np.random.default_rng(3)
    arrays = {"loss": np.array(1.25, dtype=np.float32), "hatom": rng.standard_normal((1000, 300)).astype(np.float32),
              "params": rng.standard_normal(10_000_000), "grads": rng.standard_normal(10_000_000).astype(np.float32),
              "index": np.arange(7, dtype=np.int64)}
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), arrays)
    files = sorted(glob.glob(str(tmp_path / "a" / "*.npy")))
    assert [os.path.basename(f) for f in files] == ["grads.npy", "hatom.npy", "index.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(f) for f in files) <= 64e6
    for f in files:
        x, y = np.load(f), np.load(f.replace(os.sep + "a" + os.sep, os.sep + "b" + os.sep))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert np.load(files[3]).shape == () and float(np.load(files[3])) == 1.25
    assert np.load(files[2]).dtype == np.float32 and np.array_equal(np.load(files[2]), np.arange(7))
    params = np.load(files[4])
    assert params.dtype == np.float64 and 0 < params.size < 10_000_000 and np.isin(params[:1000], arrays["params"]).all()
    # under the budget nothing is cut
    small = {"hatom": arrays["hatom"]}
    bench.write_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(str(tmp_path / "c" / "hatom.npy")), arrays["hatom"])
    # --steps is the number of timed steps: it has to be one at least
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    assert bench.parse_args(["--steps", "7", "--dump-outputs", "d"]).steps == 7


def test_bench_plain_run_measures_the_headline_row_alone():
    """``bench.py`` without ``--full`` skips every leg beside the headline row (the pass without the fixed-point hint, the
    roofline pass, the other message function / the bf16 leg, the VAE row, the configs[4] leg, the CPU baselines);
    ``--full`` runs them, and each of its ``--no-*`` options still skips its own leg."""
    import bench
    legs = ("no_full_depth", "no_roofline", "no_second_cell", "no_vae", "no_configs4", "no_cpu_baseline")
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "3"])
    assert not plain.full and all(getattr(plain, k) for k in legs)
    assert (plain.steps, plain.warmup, plain.gpus) == (5, 3, 1)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, k) for k in legs)
    some = bench.parse_args(["--full", "--no-vae", "--no-configs4"])
    assert some.no_vae and some.no_configs4 and not some.no_second_cell and not some.no_cpu_baseline


def test_atom_run_join_pays_what_is_owed_once_and_releases_it():
    """``atom_decode.AtomRun`` without a GPU (stub tensors, no node state): the first ``join`` runs ``finish``, a second
    one returns the same two tensors and does nothing else, and the closure is released after the first."""
    import weakref
    from ggpm_amd.atom_decode import AtomRun
    pooled, cand, calls = torch.zeros(3, 4), torch.ones(2, 4), []

    def finish():
        calls.append(1)

    probe = weakref.ref(finish)
    run = AtomRun(None, pooled, cand, finish)
    del finish
    assert probe() is not None
    first = run.join()
    assert calls == [1] and probe() is None
    second = run.join()
    assert calls == [1]
    assert first[0] is pooled and first[1] is cand and second[0] is pooled and second[1] is cand


def test_hand_offs_are_arguments_not_module_state():
    import inspect
    from ggpm_amd import atom_decode, fused
    from ggpm_amd.decoder import HierMPNDecoder
    from ggpm_amd.encoder import HierMPNEncoder
    assert not hasattr(fused, "NARROW") and not hasattr(atom_decode, "_PENDING")
    assert "beside" in inspect.signature(HierMPNEncoder.forward_padded).parameters
    assert "atom" in inspect.signature(HierMPNDecoder.forward).parameters
