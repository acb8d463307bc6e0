"""GPU: the clipping / parameter-group entry points of FlatAdam (ggpm_flat_sqnorm_partials, ggpm_flat_norm_finish,
ggpm_adam_step_groups; csrc/gather.hip) through ``_lib``, and FlatAdam on HierPropOptVAE.

The reference of every numeric check is torch in float64 on the CPU on the same fp32 inputs: ``clip_grad_norm_`` followed by
``torch.optim.Adam`` with ``param_groups`` over separately allocated tensors.  Bounds: parameters
``max|p - p64| <= 2e-6 max(1, max|p64|)`` after every step (the bar of test_adam_step_matches_torch_adam); norms ``<= 5e-7``
relative (fp64 accumulation, then one rounding through sqrt to fp32: at most two fp32 roundings, 1.2e-7; four ulps left); where
the coefficient is exactly 1 the grouped entry with one group gives the bits of ggpm_adam_step.
"""
import ctypes

import numpy as np
import pytest
import torch

from ggpm_amd import _lib, functional as F_
from ggpm_amd.optim import AdamGroup

pytestmark = pytest.mark.gpu

ERR_ARG = 1                          # GGPM_ERR_ARG (include/ggpm_hip.h)
P_TOL, NORM_TOL = 2e-6, 5e-7
SENTINEL = -777.0
ADAM_STRIDE = 2048 * 256 * 4         # floats one grid stride of adam_flat_k / adam_groups_k covers at their cap
# (lr, beta1, beta2, eps, weight_decay) of up to four groups: every field differs somewhere, one weight decay
HYPER = [(1e-2, 0.9, 0.999, 1e-8, 0.0), (3e-3, 0.9, 0.999, 1e-8, 0.01), (1e-3, 0.8, 0.99, 1e-8, 0.0), (2e-2, 0.9, 0.95, 1e-6, 0.0)]


def _dev():
    return torch.device("cuda:0")


def _lib_():
    return _lib.load()


def _norm_geometry():
    """(cap, threads) of the partials kernel, from its own workspace query: the cap is what a huge n asks for, and one
    workgroup covers 4 * threads floats (the first n that asks for two partials is 4 * threads + 4)."""
    lib = _lib_()
    cap = lib.ggpm_flat_sqnorm_workspace_bytes(1 << 40) // 8
    threads = next(t for t in (64, 128, 256, 512, 1024) if lib.ggpm_flat_sqnorm_workspace_bytes(4 * t + 4) == 16)
    assert lib.ggpm_flat_sqnorm_workspace_bytes(4 * threads) == 8 and lib.ggpm_flat_sqnorm_workspace_bytes(1) == 8
    return cap, threads


def _partials(x, n, ws):
    return _lib_().ggpm_flat_sqnorm_partials(F_._p(x), n, F_._p(ws), ws.numel() * 8, F_._stream())


def _finish(ws, n_partials, max_norm, out):
    return _lib_().ggpm_flat_norm_finish(F_._p(ws), n_partials, max_norm, F_._p(out), F_._stream())


def _coef(norm32: torch.Tensor, max_norm: float) -> float:
    """min(max_norm / (norm + 1e-6f), 1) in fp32 with one correctly rounded division, from the norm the kernel reported."""
    c = np.float32(max_norm) / (np.float32(float(norm32)) + np.float32(1e-6))
    return float(min(c, np.float32(1.0)))


def test_partials_and_finish_hold_the_norm_bound_at_every_size():
    """n = 1, 3, 64, 1025, 300*620+3, one float4 (and a tail) past one full grid stride at the kernel's cap, and past four
    strides (the unrolled loop), one after the other on ONE workspace: a call after a call of another size is still right, a
    second call gives the same bits, and nothing outside partials[:count] and out[:1 or 2] is written."""
    lib, dev = _lib_(), _dev()
    cap, threads = _norm_geometry()
    stride = cap * threads * 4
    sizes = [1, 3, 64, 1025, 300 * 620 + 3, stride + 7, 4 * stride + 4 * 5 + 3, 1025, 1]
    gen = torch.Generator().manual_seed(11)
    for case, n in enumerate(sizes):
        x_cpu = torch.randn(n, generator=gen) * (0.3 + case)
        if case == 3:                                    # one 1e3 entry among 1e-2 entries
            x_cpu = torch.full((n,), 1e-2)
            x_cpu[517] = 1e3
        want = float(torch.linalg.vector_norm(x_cpu.double()))
        x = x_cpu.to(dev)
        count = lib.ggpm_flat_sqnorm_workspace_bytes(n) // 8
        assert 1 <= count <= cap and count == min(cap, max(1, (n // 4 + threads - 1) // threads))
        ws = torch.full((cap + 8,), SENTINEL, dtype=torch.float64, device=dev)
        out = torch.full((6,), SENTINEL, device=dev)
        assert _partials(x, n, ws) == 0 and _finish(ws, count, 0.0, out) == 0
        got = float(out[0])
        print("n=%d count=%d norm=%.9g want=%.9g rel=%.3e" % (n, count, got, want, abs(got - want) / want))
        assert abs(got - want) <= NORM_TOL * want, (n, got, want)
        assert bool((ws[count:] == SENTINEL).all()) and bool((out[1:] == SENTINEL).all()), n
        assert abs(float(ws[:count].sum().sqrt()) - want) <= 1e-12 * want      # the partials are fp64 sums (chains of < 100 terms)
        # with a bound: torch's coefficient from the fp32 norm, once clipping and once not
        for max_norm in (0.5 * want, 2.0 * want):
            assert _finish(ws, count, max_norm, out) == 0
            assert float(out[0]) == got and bool((out[2:] == SENTINEL).all())
            assert float(out[1]) == _coef(out[0], max_norm), (n, max_norm)
            assert (float(out[1]) < 1.0) == (max_norm < want)
        ws2 = torch.full_like(ws, SENTINEL)
        out2 = torch.full_like(out, SENTINEL)
        assert _partials(x, n, ws2) == 0 and _finish(ws2, count, 0.0, out2) == 0
        assert torch.equal(ws2, ws) and float(out2[0]) == got


def test_partials_and_finish_refuse_bad_arguments_and_write_nothing():
    lib, dev = _lib_(), _dev()
    x = torch.randn(4096 + 4, device=dev)
    ws = torch.full((8,), SENTINEL, dtype=torch.float64, device=dev)
    out = torch.full((4,), SENTINEL, device=dev)
    s = F_._stream()
    need = lib.ggpm_flat_sqnorm_workspace_bytes(4100)
    assert need == 16
    assert lib.ggpm_flat_sqnorm_partials(None, 4100, F_._p(ws), 64, s) == ERR_ARG
    assert lib.ggpm_flat_sqnorm_partials(F_._p(x), 4100, None, 64, s) == ERR_ARG
    assert lib.ggpm_flat_sqnorm_partials(F_._p(x), 0, F_._p(ws), 64, s) == ERR_ARG
    assert lib.ggpm_flat_sqnorm_partials(F_._p(x[1:]), 64, F_._p(ws), 64, s) == ERR_ARG            # x not 16-byte aligned
    assert lib.ggpm_flat_sqnorm_partials(F_._p(x), 4100, F_._p(ws), need - 8, s) == ERR_ARG        # workspace too small
    assert lib.ggpm_flat_norm_finish(None, 1, 0.0, F_._p(out), s) == ERR_ARG
    assert lib.ggpm_flat_norm_finish(F_._p(ws), 1, 0.0, None, s) == ERR_ARG
    assert lib.ggpm_flat_norm_finish(F_._p(ws), 0, 0.0, F_._p(out), s) == ERR_ARG
    assert lib.ggpm_flat_norm_finish(F_._p(ws), _norm_geometry()[0] + 1, 0.0, F_._p(out), s) == ERR_ARG
    assert bool((ws == SENTINEL).all()) and bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- grouped Adam
def _tile_map(layout, ntiles):
    """(n_groups, tile -> group or None)."""
    if layout == "one":
        return 1, None
    if layout == "four":                                 # alternating per tile: one wave (four tiles) holds four groups
        return 4, torch.arange(ntiles, dtype=torch.int64) % 4
    tiles = torch.zeros(ntiles, dtype=torch.int64)        # "lone": group 1 owns ONE tile (the only one when n = 64)
    tiles[ntiles // 2] = 1
    return 2, tiles


def _groups_c(hyper, lr_scale=1.0):
    arr = (AdamGroup * len(hyper))()
    for c, (lr, b1, b2, eps, wd) in zip(arr, hyper):
        c.lr, c.beta1, c.beta2, c.eps, c.weight_decay = lr * lr_scale, b1, b2, eps, wd
    return arr


def _step_groups(p, g, m, v, tiles_dev, groups, step, ws=None, count=0, max_norm=0.0, clip_out=None, write_clipped=0, n=None):
    return _lib_().ggpm_adam_step_groups(F_._p(p), F_._p(g), F_._p(m), F_._p(v), p.numel() if n is None else n,
                                         F_._p(tiles_dev), len(groups), ctypes.addressof(groups), step, F_._p(ws), count,
                                         max_norm, F_._p(clip_out), write_clipped, F_._stream())


class _Problem:
    """p0 and six gradients (scale alternating 0.1 / 3) on the CPU, shared by the cases of one size; tile 2 is padding."""

    _cache = {}

    def __init__(self, n):
        gen = torch.Generator().manual_seed(n % 1000003)
        self.n = n
        self.p0 = torch.randn(n, generator=gen)
        self.grads = [torch.randn(n, generator=gen) * (0.1 if k % 2 == 0 else 3.0) for k in range(6)]
        if n >= 3 * 64:
            self.p0[128:192] = 0
            for g in self.grads:
                g[128:192] = 0
        self.norms = [float(torch.linalg.vector_norm(g.double())) for g in self.grads]

    @classmethod
    def get(cls, n):
        if n not in cls._cache:
            cls._cache[n] = cls(n)
        return cls._cache[n]


def _reference_run(prob, n_groups, tiles, max_norm):
    """float64 on the CPU: one separately allocated tensor per group, clip_grad_norm_, torch.optim.Adam(param_groups), an lr decay
    of 0.9 behind step 3.  Returns the flat fp64 parameters after every step and the norms clip_grad_norm_ returned."""
    idx = [torch.arange(prob.n)] if tiles is None else [
        (tiles.repeat_interleave(64) == k).nonzero().reshape(-1) for k in range(n_groups)]
    ps = [torch.nn.Parameter(prob.p0.double()[i].clone()) for i in idx]
    opt = torch.optim.Adam([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                            for q, h in zip(ps, HYPER)])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9)
    after, norms = [], []
    for k, g in enumerate(prob.grads):
        for q, i in zip(ps, idx):
            q.grad = g.double()[i].clone()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
        if k == 2:
            sched.step()
        flat = torch.empty(prob.n, dtype=torch.float64)
        for q, i in zip(ps, idx):
            flat[i] = q.detach()
        after.append(flat)
    return after, norms


@pytest.mark.parametrize("mode", ["clipping", "not_clipping", "no_partials"])
@pytest.mark.parametrize("layout", ["one", "four", "lone"])
@pytest.mark.parametrize("n", [64, 64 * 7, ADAM_STRIDE + 64 * 5])
def test_grouped_adam_six_steps_against_float64(n, layout, mode):
    dev = _dev()
    lib = _lib_()
    prob = _Problem.get(n)
    n_groups, tiles = _tile_map(layout, n // 64)
    max_norm = {"clipping": 0.5 * min(prob.norms), "not_clipping": 2.0 * max(prob.norms), "no_partials": None}[mode]
    want, ref_norms = _reference_run(prob, n_groups, tiles, max_norm)
    if mode == "clipping":
        assert all(r > max_norm for r in ref_norms)
    elif mode == "not_clipping":
        assert all(r < max_norm for r in ref_norms)
    p, m, v = prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    tiles_dev = None if tiles is None else tiles.to(torch.uint8).to(dev)
    count = lib.ggpm_flat_sqnorm_workspace_bytes(n) // 8
    ws = torch.zeros(count, dtype=torch.float64, device=dev)
    clip_out = torch.full((4,), SENTINEL, device=dev)
    for k, g_cpu in enumerate(prob.grads):
        g = g_cpu.to(dev)
        groups = _groups_c(HYPER[:n_groups], 0.9 if k >= 3 else 1.0)
        if max_norm is None:
            assert _step_groups(p, g, m, v, tiles_dev, groups, k + 1) == 0
        else:
            assert _partials(g, n, ws) == 0
            assert _step_groups(p, g, m, v, tiles_dev, groups, k + 1, ws, count, max_norm, clip_out) == 0
            norm, coef = float(clip_out[0]), float(clip_out[1])
            assert abs(norm - ref_norms[k]) <= NORM_TOL * ref_norms[k], (k, norm, ref_norms[k])
            assert coef == _coef(clip_out[0], max_norm) and (coef < 1.0) == (mode == "clipping")
            assert bool((clip_out[2:] == SENTINEL).all())
        assert torch.equal(g.cpu(), g_cpu)               # without write_clipped the gradient is left as it was
        err = float((p.cpu().double() - want[k]).abs().max())
        bound = P_TOL * max(1.0, float(want[k].abs().max()))
        print("n=%d %s %s step %d: err %.3e bound %.3e" % (n, layout, mode, k + 1, err, bound))
        assert err <= bound, (k, err, bound)
    if n >= 3 * 64:                                      # the padding tile stayed zero under its group's weight decay too
        assert not bool(p[128:192].any()) and not bool(m[128:192].any()) and not bool(v[128:192].any())


@pytest.mark.parametrize("n", [64 * 7, ADAM_STRIDE + 64 * 5])
def test_one_group_with_coefficient_one_gives_the_bits_of_adam_step(n):
    """ggpm_adam_step_groups with one group and a null map against ggpm_adam_step, three steps with weight decay: with null
    partials, and with partials under a bound far above the norm (coefficient exactly 1)."""
    dev, lib = _dev(), _lib_()
    prob = _Problem.get(n)
    lr, b1, b2, eps, wd = HYPER[1]
    count = lib.ggpm_flat_sqnorm_workspace_bytes(n) // 8
    ws = torch.zeros(count, dtype=torch.float64, device=dev)
    clip_out = torch.zeros(2, device=dev)
    state = [[prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)] for _ in range(3)]
    groups = _groups_c([HYPER[1]])
    for k in range(3):
        g = prob.grads[k].to(dev)
        p, m, v = state[0]
        assert lib.ggpm_adam_step(F_._p(p), F_._p(g), F_._p(m), F_._p(v), n, lr, b1, b2, eps, wd, k + 1, F_._stream()) == 0
        assert _step_groups(state[1][0], g, state[1][1], state[1][2], None, groups, k + 1) == 0
        assert _partials(g, n, ws) == 0
        assert _step_groups(state[2][0], g, state[2][1], state[2][2], None, groups, k + 1, ws, count, 1e9, clip_out, 1) == 0
        assert float(clip_out[1]) == 1.0 and torch.equal(g.cpu(), prob.grads[k])
    for other in state[1:]:
        for a, b in zip(state[0], other):
            assert torch.equal(a, b)


def test_write_clipped_stores_the_scaled_gradient_and_changes_nothing_else():
    dev = _dev()
    n = 64 * 7
    prob = _Problem.get(n)
    n_groups, tiles = _tile_map("four", n // 64)
    tiles_dev = tiles.to(torch.uint8).to(dev)
    groups = _groups_c(HYPER)
    max_norm = 0.5 * prob.norms[0]
    runs = []
    for write in (0, 1):
        p, m, v, g = prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), prob.grads[0].to(dev)
        ws = torch.zeros(1, dtype=torch.float64, device=dev)
        clip_out = torch.zeros(2, device=dev)
        assert _partials(g, n, ws) == 0
        assert _step_groups(p, g, m, v, tiles_dev, groups, 1, ws, 1, max_norm, clip_out, write) == 0
        runs.append((p, m, v, g, clip_out))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][:3], runs[1][:3])) and torch.equal(runs[0][4], runs[1][4])
    g0 = prob.grads[0].to(dev)
    assert torch.equal(runs[0][3], g0)
    assert 0.0 < float(runs[1][4][1]) < 1.0
    assert torch.equal(runs[1][3], g0 * runs[1][4][1])               # the bits of g * coef with the coefficient reported


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_propagates_as_under_clip_grad_norm(bad):
    """One Inf element: coefficient 0, NaN in that element alone; a NaN: NaN everywhere.  isnan masks of p and g against
    torch's clip_grad_norm_ (error_if_nonfinite=False) + Adam on the device, one tensor per group."""
    dev = _dev()
    n = 64 * 7
    prob = _Problem.get(n)
    n_groups, tiles = _tile_map("four", n // 64)
    g_cpu = prob.grads[1].clone()
    g_cpu[200] = bad
    idx = [(tiles.repeat_interleave(64) == k).nonzero().reshape(-1).to(dev) for k in range(n_groups)]
    ps = [torch.nn.Parameter(prob.p0.to(dev)[i].clone()) for i in idx]
    opt = torch.optim.Adam([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                            for q, h in zip(ps, HYPER)])
    for q, i in zip(ps, idx):
        q.grad = g_cpu.to(dev)[i].clone()
    torch.nn.utils.clip_grad_norm_(ps, 1.0)
    opt.step()
    want_p, want_g = torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    for q, i in zip(ps, idx):
        want_p[i], want_g[i] = q.detach().isnan(), q.grad.isnan()
    p, m, v, g = prob.p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), g_cpu.to(dev)
    ws = torch.zeros(1, dtype=torch.float64, device=dev)
    clip_out = torch.zeros(2, device=dev)
    assert _partials(g, n, ws) == 0
    assert _step_groups(p, g, m, v, tiles.to(torch.uint8).to(dev), _groups_c(HYPER), 1, ws, 1, 1.0, clip_out, 1) == 0
    assert torch.equal(p.isnan(), want_p) and torch.equal(g.isnan(), want_g)
    assert int(want_p.sum()) == (1 if bad == float("inf") else n)
    if bad == float("inf"):
        assert float(clip_out[0]) == float("inf") and float(clip_out[1]) == 0.0


def test_grouped_adam_refuses_bad_arguments_and_writes_nothing():
    dev, lib = _dev(), _lib_()
    n = 64 * 4
    bufs = [torch.randn(n + 4, device=dev) for _ in range(4)]
    p, g, m, v = (b[:n] for b in bufs)
    before = [b.clone() for b in bufs]
    tiles = (torch.arange(n // 64) % 2).to(torch.uint8).to(dev)
    ws = torch.ones(4, dtype=torch.float64, device=dev)
    clip_out = torch.full((2,), SENTINEL, device=dev)
    two, nine = _groups_c(HYPER[:2]), (AdamGroup * 9)()
    ok = dict(tiles_dev=tiles, groups=two, step=1, ws=ws, count=1, max_norm=1.0, clip_out=clip_out)

    def call(p=p, g=g, m=m, v=v, n=n, **kw):
        a = dict(ok, **kw)
        return _step_groups(p, g, m, v, a["tiles_dev"], a["groups"], a["step"], a["ws"], a["count"], a["max_norm"],
                            a["clip_out"], 1, n=n)

    s = F_._stream()
    for i in range(4):                                   # each of p, g, m, v null, then misaligned
        args = [p, g, m, v]
        args[i] = None
        assert lib.ggpm_adam_step_groups(*(F_._p(t) for t in args), n, F_._p(tiles), 2, ctypes.addressof(two), 1, None, 0, 0.0,
                                         None, 0, s) == ERR_ARG
        args[i] = bufs[i][1:n + 1]
        assert call(*args) == ERR_ARG
    assert lib.ggpm_adam_step_groups(F_._p(p), F_._p(g), F_._p(m), F_._p(v), n, F_._p(tiles), 2, None, 1, None, 0, 0.0, None,
                                     0, s) == ERR_ARG                                   # no hyper-parameters
    assert call(n=0) == ERR_ARG and call(n=n - 4) == ERR_ARG and call(n=n - 32) == ERR_ARG
    for n_groups in (0, 9, -1):
        assert lib.ggpm_adam_step_groups(F_._p(p), F_._p(g), F_._p(m), F_._p(v), n, F_._p(tiles), n_groups,
                                         ctypes.addressof(nine), 1, None, 0, 0.0, None, 0, s) == ERR_ARG
    assert call(tiles_dev=None) == ERR_ARG               # two groups and no map
    assert call(step=0) == ERR_ARG and call(step=-3) == ERR_ARG
    for bad in (0.0, -1.0, float("nan")):
        assert call(max_norm=bad) == ERR_ARG
    assert call(count=0) == ERR_ARG and call(count=_norm_geometry()[0] + 1) == ERR_ARG
    assert bool((clip_out == SENTINEL).all())
    for b, was in zip(bufs, before):
        assert torch.equal(b, was)


# ---------------------------------------------------------------------------------------------- model level
class _CountingLib:
    """libggpm_hip behind a proxy that records the name of every entry point called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def _four_groups(model, lrs):
    """The split of vae_fine_tune_indv_opt.py:61-70 by the same name tests: the rest, 'decoder', 'homo_linear', 'lumo_linear'."""
    named = list(model.named_parameters())
    keys = ("decoder", "homo_linear", "lumo_linear")
    sets = [[p for k, p in named if not any(key in k for key in keys)]] + [[p for k, p in named if key in k] for key in keys]
    assert all(sets) and sum(len(s) for s in sets) == len(named)
    return [{"params": s, "lr": lr} for s, lr in zip(sets, lrs)]


@pytest.mark.parametrize("which", ["below", "above"])
def test_flat_adam_on_hierpropoptvae_matches_clip_grad_norm_and_four_adams(which, monkeypatch):
    """Four steps of zero_grad -> forward -> backward -> sync.all_reduce() -> step(clip_norm=c) against a twin from the same
    weights driven by clip_grad_norm_ + four torch.optim.Adam; c once below and once above all four norms (asserted on the
    twin).  The step and the two norms run under set_sync_debug_mode("error"), and a clipped step is two library calls.

    The twin's own backward gives the model's gradients bit for bit only while their parameters are equal, which is the first
    step: behind it the two differ in last bits (torch's fused Adam against this kernel, both inside the bound), and Adam's
    m / (sqrt(v) + eps) turns a last-bit change of a gradient near eps into a change of order lr (measured: 3.1e-4 after the
    second unclipped step).  So the first step asserts that the twin's gradients ARE the model's, and every step hands the
    twin the model's gradients: the same fp32 inputs on both sides, as in the kernel-level tests."""
    import property_fixtures as pf
    from test_property_gpu import _propopt_model, _step
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    g = pf.PropOptGolden(pf.names("propopt")[0])
    lrs = (1e-3, 5e-4, 2e-3, 3e-3)
    model, tensors, sch = _propopt_model(g)
    twin, _, _ = _propopt_model(g)
    twin_opts = [torch.optim.Adam(grp["params"], lr=grp["lr"]) for grp in _four_groups(twin, lrs)]
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    opt = FlatAdam(sync, lr=1e-3, param_groups=_four_groups(model, lrs))
    assert opt._hip and len(opt.param_groups) == 4
    clip = {"below": 1e-3, "above": 1e6}[which]
    for step in range(4):
        opt.zero_grad()
        _step(g, model, tensors, sch)[0].backward()
        sync.all_reduce()
        if step == 0:                                    # equal parameters: the twin's own backward gives the same bits
            twin.zero_grad()
            _step(g, twin, tensors, sch)[0].backward()
            for p, q in zip(model.parameters(), twin.parameters()):
                assert torch.equal(p.grad, q.grad) if q.grad is not None else not bool(p.grad.any())
        for p, q in zip(model.parameters(), twin.parameters()):
            q.grad = p.grad.detach().clone()
        want_gn = float(torch.sqrt(sum(q.grad.double().pow(2).sum() for q in twin.parameters())))
        twin_norm = float(torch.nn.utils.clip_grad_norm_(twin.parameters(), clip))
        assert twin_norm > clip if which == "below" else twin_norm < clip, (step, twin_norm)
        for o in twin_opts:
            o.step()
        want_pn = float(torch.sqrt(sum(p.detach().double().pow(2).sum() for p in model.parameters())))
        counting = _CountingLib(_lib.load())
        monkeypatch.setattr(_lib, "_LIB", counting)
        torch.cuda.set_sync_debug_mode("error")
        try:
            gn, pn = opt.grad_norm(), opt.param_norm()
            assert counting.calls == ["ggpm_flat_sqnorm_partials", "ggpm_flat_norm_finish"] * 2
            del counting.calls[:]
            opt.step(clip_norm=clip)
            assert counting.calls == ["ggpm_flat_sqnorm_partials", "ggpm_adam_step_groups"]
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.undo()
        assert gn.dim() == 0 and pn.dim() == 0 and opt.last_grad_norm.dim() == 0 and gn.is_cuda
        norm = float(opt.last_grad_norm)
        print("step %d: norm %.9g twin %.9g; grad_norm %.9g param_norm %.9g (%.9g)" % (step, norm, twin_norm, float(gn), float(pn),
                                                                                      want_pn))
        assert float(gn) == norm                             # the same partials in the same order
        assert abs(float(pn) - want_pn) <= NORM_TOL * want_pn
        assert abs(norm - want_gn) <= NORM_TOL * want_gn     # (want_gn: the twin's gradients before its clip, summed in fp64)
        assert (float(opt.last_clip_coef) < 1.0) == (which == "below")
        ps, qs = list(model.parameters()), list(twin.parameters())
        err = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(ps, qs))
        bound = P_TOL * max(1.0, max(float(q.detach().abs().max()) for q in qs))
        print("step %d: parameters err %.3e bound %.3e" % (step, err, bound))
        assert err <= bound, (step, err, bound)


def test_default_flat_adam_step_is_still_one_adam_step_launch(monkeypatch):
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 1), torch.nn.Linear(1, 7)).to(_dev())
    sync = FlatGradSync(model.parameters(), keep_flat=True)
    opt = FlatAdam(sync, lr=1e-2)
    model(torch.randn(3, 5, device=_dev())).sum().backward()
    sync.all_reduce()
    counting = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_LIB", counting)
    opt.step()
    assert counting.calls == ["ggpm_adam_step"]


@pytest.mark.parametrize("hip", [True, False])
def test_flat_adam_wrapper_in_both_forms_against_float64(hip, monkeypatch):
    """FlatAdam itself on the device with random gradients, four groups, clip_norm = 20 (clipping on the large-gradient steps
    only), an ExponentialLR step in the middle: the HIP form (with write_clipped: p.grad reads as clip_grad_norm_ leaves it)
    and the torch-op form (_dev.HIP_ADAM off, the A/B partner) against clip_grad_norm_ + torch.optim.Adam in float64."""
    from ggpm_amd import _dev as dev_switches
    from ggpm_amd.optim import FlatAdam
    from ggpm_amd.parallel import FlatGradSync
    monkeypatch.setattr(dev_switches, "HIP_ADAM", hip)
    dev = _dev()
    gen = torch.Generator().manual_seed(7)
    sizes = [(1,), (7,), (64,), (30, 62), (4096,), (63,), (65,), (1000,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in sizes]
    hyper = [{"lr": 1e-2}, {"lr": 3e-3, "weight_decay": 0.01}, {"lr": 1e-3, "betas": (0.8, 0.99)}, {"lr": 2e-2, "eps": 1e-6}]
    twins = [torch.nn.Parameter(p.detach().cpu().double()) for p in params]
    ref_opt = torch.optim.Adam([dict(h, params=twins[k::4]) for k, h in enumerate(hyper)])
    sync = FlatGradSync(params, keep_flat=True)
    opt = FlatAdam(sync, param_groups=[dict(h, params=params[k::4]) for k, h in enumerate(hyper)])
    assert opt._hip == hip
    scheds = [torch.optim.lr_scheduler.ExponentialLR(o, 0.9) for o in (opt.opt, ref_opt)]
    clipped_steps = 0
    for step in range(6):
        opt.zero_grad()
        for p, q in zip(params, twins):
            g = torch.randn(p.shape, generator=gen) * (0.02 if step % 3 == 0 else 3.0)
            p.grad, q.grad = g.to(dev), g.double()
        sync.all_reduce()
        ref_norm = float(torch.nn.utils.clip_grad_norm_(twins, 20.0))
        clipped_steps += ref_norm > 20.0
        ref_opt.step()
        opt.step(clip_norm=20.0, write_clipped=True)
        if hip:
            assert abs(float(opt.last_grad_norm) - ref_norm) <= NORM_TOL * ref_norm
            # g * coef: the coefficient carries the norm's error and one rounding of its division, the product one more
            for p, q in zip(params, twins):
                assert float((p.grad.cpu().double() - q.grad).abs().max()) <= (NORM_TOL + 2.4e-7) * float(q.grad.abs().max())
        big = max(float(q.detach().abs().max()) for q in twins)
        err = max(float((p.detach().cpu().double() - q.detach()).abs().max()) for p, q in zip(params, twins))
        print("hip=%s step %d: norm %.9g (ref %.9g) err %.3e bound %.3e" % (hip, step, float(opt.last_grad_norm), ref_norm, err,
                                                                             P_TOL * max(1.0, big)))
        assert err <= P_TOL * max(1.0, big), (step, err)
        if step == 2:
            for s in scheds:
                s.step()
    assert clipped_steps == 4
