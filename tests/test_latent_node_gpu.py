"""GPU: the one latent-terms node (ggpm_amd.latent_heads._LatentTerms) under every variant of ``bound_loss``
(ggpm_amd.objectives.VARIANTS), one output at a time.  The end-to-end tests drive every output of the node at once; here each
output alone receives a random cotangent, so an upstream gradient that did not arrive, an addition made although nothing
arrived for it, or a variant that saves the wrong tensors shows.

The yardstick is ``restate``: the node's outputs written once more in torch fp64 on the CPU and differentiated by autograd --
the latent terms of tests/likelihood_oracle.py, the free-bits term of tests/latent_dims_oracle.py, the split of
tests/latent_decomp_oracle.py and, for the path variants, the stop-gradient form tests/mol_estimator_oracle.py restates
(log q with the posterior's parameters detached, kl taking no part, for DReG the gradient at z_k weighted by s_k once more).
PARITY = 1e-4, norm-wise (golden_utils.rel_err), as in BASELINE.json and the end-to-end tests of these quantities; where the
fp64 gradient is exactly zero the node must return exact zeros or None.  Every third latent column has tiny head weights, so
its batch-mean KL is below ``free_bits`` and the free-bits term leaves its rows of R_mean / R_var without gradient."""
import functools
import math

import numpy as np
import pytest
import torch

from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = 1e-4
SHAPES = [(2, 3, 5, 6), (3, 5, 70, 9)]          # (K, B, L, H); 70 latent columns cross one 64-lane wave
N_DATA, FREE_BITS = 50, 0.05
INPUTS = ("z_vecs", "Wm", "bm", "Wv", "bv")
# per entry of VARIANTS: the arguments of bound_loss that select it, the names of its further outputs, how many tensors its
# node saves (a variant that is not listed here fails the tests: add it)
ARGS = {"plain": dict(objective="elbo"), "free_bits": dict(objective="elbo", free_bits=FREE_BITS),
        "tcvae": dict(objective="tcvae", dataset_size=N_DATA), "stl": dict(objective="iwae"), "dreg": dict(objective="iwae")}
EXTRAS = {"plain": (), "free_bits": ("term", "kl_dims"), "tcvae": ("comps",), "stl": (), "dreg": ()}
SAVED = {"plain": 6, "free_bits": 7, "tcvae": 9, "stl": 6, "dreg": 6}


def _modes():
    from ggpm_amd.objectives import VARIANTS
    return sorted(VARIANTS)


@pytest.fixture(autouse=True)
def _gradients_as_return_values(monkeypatch):
    monkeypatch.setenv("GGPM_SIDE_STREAM", "0")


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """fp32 numpy: z_vecs [B, H], the heads, eps [K, B, L], the DReG weights s [K, B] and one cotangent per output"""
    K, B, L, H = shape
    rs = np.random.RandomState(1000 + L)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    d = dict(z_vecs=f(B, H), Wm=0.5 * f(L, H), bm=0.5 * f(L), Wv=0.5 * f(L, H), bv=0.5 * f(L), eps=f(K, B, L))
    for k in ("Wm", "bm", "Wv", "bv"):
        d[k][::3] *= np.float32(1e-2)
    e = np.exp(f(K, B))
    d["s"] = (e / e.sum(axis=0)[None]).astype(np.float32)
    d["cot"] = dict(z=f(K, B, L), kl=f(B), logpq=f(K, B), term=f(), comps=f(K, B, 3))
    return d


def restate(mode, d):
    """-> (the five inputs as fp64 leaves, the node's outputs by name in fp64, (mean, pre_var))"""
    t = {k: torch.tensor(d[k].astype(np.float64), requires_grad=k in INPUTS) for k in INPUTS + ("eps", "s")}
    eps, path = t["eps"], mode in ("stl", "dreg")
    K, B, L = eps.shape
    mean, pv = t["z_vecs"] @ t["Wm"].T + t["bm"], t["z_vecs"] @ t["Wv"].T + t["bv"]
    lv = -pv.abs()
    z = mean[None] + torch.exp(lv / 2)[None] * eps
    if mode == "dreg":
        z.register_hook(lambda g: g * t["s"][:, :, None])
    kl_dim = -0.5 * (1.0 + lv - mean * mean - torch.exp(lv))
    out = dict(z=z, kl=kl_dim.sum(dim=1).detach() if path else kl_dim.sum(dim=1))
    if path:
        m0, lv0 = mean.detach(), lv.detach()
        out["logpq"] = -0.5 * (z * z).sum(dim=2) + 0.5 * ((z - m0[None]) ** 2 * torch.exp(-lv0)[None] + lv0[None]).sum(dim=2)
    else:
        out["logpq"] = -0.5 * (z * z).sum(dim=2) + 0.5 * (eps * eps + lv[None]).sum(dim=2)
    if mode == "free_bits":
        out["kl_dims"] = kl_dim.mean(dim=0)
        out["term"] = torch.maximum(out["kl_dims"], torch.tensor(FREE_BITS, dtype=torch.float64)).sum()
        out["kl_dims"] = out["kl_dims"].detach()
    if mode == "tcvae":
        c, l2pi = math.log(float(N_DATA) * B), math.log(2.0 * math.pi)
        e = -0.5 * (l2pi + lv[None, None] + (z[:, :, None, :] - mean[None, None]) ** 2 * torch.exp(-lv)[None, None])
        S = e.sum(dim=3)
        A, D = torch.logsumexp(S, dim=2), torch.logsumexp(e, dim=2).sum(dim=2)
        logp = (-0.5 * (l2pi + z * z)).sum(dim=2)
        out["comps"] = torch.stack([torch.diagonal(S, dim1=1, dim2=2) - A + c, A - D + (L - 1) * c, D - L * c - logp], dim=-1)
    return [t[k] for k in INPUTS], out, (mean, pv)


def _grads(leaves, outs, cots):
    g = torch.autograd.grad(outs, leaves, cots, allow_unused=True, retain_graph=True)
    return [None if v is None else v.detach().cpu().numpy().astype(np.float64) for v in g]


@functools.lru_cache(maxsize=None)
def want(mode, shape):
    """fp64: (outputs by name, {name of a differentiable output: the five gradients when it alone is driven}, the five when
    all are); an output that takes no part in the restatement (kl of the path variants) gives None five times"""
    d = inputs(shape)
    leaves, out, _ = restate(mode, d)
    cot = {k: torch.tensor(d["cot"][k].astype(np.float64)) for k in out if k != "kl_dims"}
    live = [k for k in cot if out[k].requires_grad]
    single = {k: _grads(leaves, [out[k]], [cot[k]]) if k in live else [None] * len(INPUTS) for k in cot}
    return ({k: v.detach().numpy() for k, v in out.items()}, single,
            _grads(leaves, [out[k] for k in live], [cot[k] for k in live]))


def node(mode, shape, params=False):
    """The node on the GPU -> (the five inputs as fp32 leaves, its outputs by name)"""
    from ggpm_amd.latent_heads import _LatentTerms
    from ggpm_amd.objectives import VARIANTS
    K, B, L, H = shape
    d = inputs(shape)
    kw = dict(objective=None, beta=1.0, alpha=None, gamma=None, dataset_size=None, free_bits=None)
    kw.update(ARGS[mode])
    variant = VARIANTS[mode]("test", B, L, **kw)
    if hasattr(variant, "s"):
        variant.s = torch.tensor(d["s"], device=DEV)
    leaves = [torch.tensor(d[k], device=DEV, requires_grad=True) for k in INPUTS]
    if params:
        leaves[1:] = [torch.nn.Parameter(v.detach()) for v in leaves[1:]]
    outs = _LatentTerms.apply(*leaves, torch.tensor(d["eps"], device=DEV), variant)
    names = ("z", "kl", "logpq") + EXTRAS[mode]
    assert len(outs) == len(names) and len(outs[0].grad_fn.saved_tensors) == SAVED[mode]
    return leaves, dict(zip(names, outs))


def _close(got, ref, what):
    """``got`` (a tensor or None) against the fp64 ``ref`` (an array or None)"""
    if ref is None or not ref.any():
        assert got is None or not got.any(), (what, "must be exact zeros or None")
        return 0.0
    assert got is not None, what
    got = got.detach().cpu().numpy().astype(np.float64)
    e = rel_err(got, ref)
    print("%s: distance %.3e" % (what, e))
    assert e < PARITY, (what, e)
    assert not got[ref == 0.0].any(), (what, "elements that are exactly zero in fp64")
    return e


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", _modes())
def test_forward_outputs(mode, shape):
    ref = want(mode, shape)[0]
    _, out = node(mode, shape)
    assert set(out) == set(ref)
    for k, v in out.items():
        assert v.dtype == torch.float32 and v.shape == ref[k].shape, (k, v.shape, ref[k].shape)
        _close(v, ref[k], "%s %s output %s" % (mode, shape, k))
    assert [k for k, v in out.items() if not v.requires_grad] == [k for k in out if k == "kl_dims"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", _modes())
def test_each_output_driven_alone_and_all_together(mode, shape):
    _, single, together = want(mode, shape)
    cot = {k: torch.tensor(v, device=DEV) for k, v in inputs(shape)["cot"].items()}
    total = [None] * len(INPUTS)
    for k, ref in single.items():
        leaves, out = node(mode, shape)
        got = torch.autograd.grad([out[k]], leaves, [cot[k]], allow_unused=True)
        for i, name in enumerate(INPUTS):
            _close(got[i], ref[i], "%s %s d%s from %s alone" % (mode, shape, name, k))
            if got[i] is not None:
                total[i] = got[i].double() if total[i] is None else total[i] + got[i].double()
    leaves, out = node(mode, shape)
    got = torch.autograd.grad([out[k] for k in single], leaves, [cot[k] for k in single], allow_unused=True)
    for i, name in enumerate(INPUTS):
        _close(got[i], together[i], "%s %s d%s from all outputs" % (mode, shape, name))
        _close(got[i], None if total[i] is None else total[i].cpu().numpy(), "%s %s d%s against the sum of the single ones"
               % (mode, shape, name))


@pytest.mark.parametrize("mode", ["stl", "dreg"])
def test_path_variant_refuses_a_second_backward(mode):
    shape = SHAPES[0]
    leaves, out = node(mode, shape)
    cot = torch.tensor(inputs(shape)["cot"]["logpq"], device=DEV)
    torch.autograd.grad([out["logpq"]], leaves, [cot], allow_unused=True, retain_graph=True)
    with pytest.raises(RuntimeError, match="path latent terms: a retained graph is not supported"):
        torch.autograd.grad([out["logpq"]], leaves, [cot], allow_unused=True)


@pytest.mark.parametrize("mode", _modes())
def test_published_gradients_on_the_second_stream(mode, monkeypatch):
    """GGPM_SIDE_STREAM on: the four head gradients are written to ``.grad`` on the second stream, d(z_vecs) comes back
    through autograd"""
    monkeypatch.setenv("GGPM_SIDE_STREAM", "1")
    shape = SHAPES[1]
    _, single, together = want(mode, shape)
    cot = inputs(shape)["cot"]
    leaves, out = node(mode, shape, params=True)
    sum((out[k] * torch.tensor(cot[k], device=DEV)).sum() for k in single).backward()
    torch.cuda.synchronize()
    for i, name in enumerate(INPUTS):
        _close(leaves[i].grad, together[i], "%s %s d%s in .grad" % (mode, shape, name))
