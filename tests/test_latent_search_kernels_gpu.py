"""GPU: the two entry points of csrc/latent_search.hip, called directly, against tests/latent_search_oracle.py at the shapes
of tests/latent_search_cases.py (whose conditions -- decision margins of 1e-4 in the fp64 run, the same decisions in fp32 --
tests/test_latent_search_oracle_cpu.py holds without a GPU).  Bound, per element of z_out, pred, terms and J:
max(1e-4, 4 |oracle fp32 - oracle fp64|) around the oracle's fp32 run; steps_taken exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import latent_search_cases as lc
import latent_search_oracle as lso

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    from ggpm_amd import functional as F_
    return F_._stream()


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def head_struct(layers):
    """ggpm_prop_head over device copies of (W, b) -> (struct, the tensors that keep its pointers alive)"""
    from ggpm_amd.property import PropHeadC
    s, keep = PropHeadC(), []
    s.n_linear = len(layers)
    s.width[0] = layers[0][0].shape[1]
    for i, (W, b) in enumerate(layers):
        Wd, bd = _dev(W), _dev(b)
        keep += [Wd, bd]
        s.width[i + 1], s.W[i], s.b[i] = W.shape[0], Wd.data_ptr(), bd.data_ptr()
    return s, keep


def guided(x, half, K, B, lr, momentum, steps, delta, w, aw, pw, expect=OK, over=None):
    """ggpm_latent_search_guided on the inputs dict ``x`` (numpy) -> dict of device tensors (outputs pre-filled with 7);
    ``over`` replaces arguments of the call by name"""
    from ggpm_amd import _lib
    hs, keep_h = head_struct(x["homo"])
    ls, keep_l = head_struct(x["lumo"])
    z0, mu, lv, th, tl = (_dev(x[k]) for k in ("z0", "mu", "lv", "t_h", "t_l"))
    prior = [None] * 3 if x["prior"] is None else [_dev(p) for p in x["prior"]]
    C = 0 if x["prior"] is None else x["prior"][0].shape[0]
    R, ld = z0.shape
    out = dict(z=torch.full((R, ld), 7.0, device=DEV), pred=torch.full((2, R), 7.0, device=DEV),
               terms=torch.full((R, 3), 7.0, device=DEV), J=torch.full((R,), 7.0, device=DEV),
               steps=torch.full((R,), 7, dtype=torch.int32, device=DEV))
    a = dict(K=K, B=B, z0=P(z0), ld=ld, half=half, mu=P(mu), lv=P(lv), homo=ctypes.byref(hs), lumo=ctypes.byref(ls), th=P(th),
             tl=P(tl), logits=P(prior[0]), means=P(prior[1]), log_vars=P(prior[2]), C=C, lr=lr, momentum=momentum, steps=steps,
             delta=delta, w_h=w[0], w_l=w[1], aw=aw, pw=pw, z_out=P(out["z"]), pred=P(out["pred"]), terms=P(out["terms"]),
             J=P(out["J"]), n=P(out["steps"]), stream=_stream())
    a.update(over or {})
    code = _lib.load().ggpm_latent_search_guided(*a.values())
    torch.cuda.synchronize()
    assert code == expect, (code, expect)
    del keep_h, keep_l
    return out


def run_case(name, molecule=None, expect=OK, **over):
    half, _, _, B, K, _, _, steps, delta, mom, aw, pw, lr, w, _, _ = lc.CASES[name]
    x = dict(lc.reference(name)[0])
    if molecule is not None:
        x["z0"] = x["z0"].reshape(K, B, -1)[:, molecule:molecule + 1].reshape(K, -1)
        for k in ("mu", "lv", "t_h", "t_l"):
            x[k] = x[k][molecule:molecule + 1]
        B = 1
    return guided(x, half, K, B, lr, mom, steps, delta, w, aw, pw, expect=expect, over=over)


@functools.lru_cache(maxsize=None)
def device_run(name):
    return {k: v.cpu().numpy() for k, v in run_case(name).items()}


@pytest.mark.parametrize("name", lc.ORDER)
def test_guided_search_matches_the_oracle(name):
    half, extra = lc.CASES[name][0], lc.CASES[name][5]
    x, r32, r64, m32, m64 = lc.reference(name)
    assert m64.min >= lc.MIN_MARGIN and m32.same_decisions(m64)
    got, bound = device_run(name), lc.bounds(r32, r64)
    assert (got["steps"] == r32["steps"]).all(), (got["steps"].tolist(), r32["steps"].tolist())
    for k in ("z", "pred", "terms", "J"):
        err = np.abs(got[k].astype(np.float64) - r32[k].astype(np.float64))
        print("%s %s: worst error %.3e, worst error / bound %.3f" % (name, k, err.max(), (err / bound[k]).max()))
        assert (err <= bound[k]).all(), "%s: worst excess %.3e" % (k, (err - bound[k]).max())
    if extra:
        assert (got["z"][:, 2 * half:] == x["z0"][:, 2 * half:]).all()


@pytest.mark.parametrize("name", ["half70_depths", "half130_c130", "delta_mid"])
def test_two_runs_are_bitwise_equal(name):
    again = run_case(name)
    for k, v in device_run(name).items():
        assert (again[k].cpu().numpy().view(np.int32) == v.view(np.int32)).all(), k


@pytest.mark.parametrize("name", ["half70_depths", "delta_mid"])
def test_a_molecule_alone_gives_the_rows_it_gives_inside_the_batch(name):
    B, K = lc.CASES[name][3], lc.CASES[name][4]
    whole = device_run(name)
    for b in (0, B - 1):
        alone = {k: v.cpu().numpy() for k, v in run_case(name, molecule=b).items()}
        rows = [k * B + b for k in range(K)]
        for key in ("z", "terms", "J", "steps"):
            assert (alone[key].view(np.int32) == whole[key][rows].view(np.int32)).all(), (b, key)
        assert (alone["pred"].view(np.int32) == whole["pred"][:, rows].view(np.int32)).all(), b


# ------------------------------------------------------------------------------------------ selection
def select(J, z, pred, terms, K, B, expect=OK, over=None):
    from ggpm_amd import _lib
    ld = z.shape[1]
    out = dict(best=torch.full((B,), 7, dtype=torch.int32, device=DEV), z=torch.full((B, ld), 7.0, device=DEV),
               pred=torch.full((2, B), 7.0, device=DEV), terms=torch.full((B, 3), 7.0, device=DEV))
    a = dict(J=P(J), z=P(z), pred=P(pred), terms=P(terms), K=K, B=B, ld=ld, best=P(out["best"]), zb=P(out["z"]),
             pb=P(out["pred"]), tb=P(out["terms"]), stream=_stream())
    a.update(over or {})
    code = _lib.load().ggpm_latent_search_select(*a.values())
    torch.cuda.synchronize()
    assert code == expect, (code, expect)
    return out


def _select_case(J):
    K, B = J.shape
    rs = np.random.RandomState(K * 100 + B)
    z, pred, terms = rs.standard_normal((K * B, 5)), rs.standard_normal((2, K * B)), rs.standard_normal((K * B, 3))
    out = select(_dev(J.reshape(-1)), _dev(z), _dev(pred), _dev(terms), K, B)
    best = lso.select(J.reshape(-1), K, B)
    rows = best * B + np.arange(B)
    assert out["best"].cpu().tolist() == best.tolist()
    assert (out["z"].cpu().numpy() == z[rows].astype(np.float32)).all()
    assert (out["pred"].cpu().numpy() == pred[:, rows].astype(np.float32)).all()
    assert (out["terms"].cpu().numpy() == terms[rows].astype(np.float32)).all()
    return best


def test_selection_ties_nan_rows_and_one_start():
    nan, inf = np.nan, np.inf
    J = np.array([[2.0, 1.0, nan, nan, inf, -inf, 5.0],
                  [1.0, 1.0, 3.0, nan, nan, nan, 5.0],
                  [1.0, 0.5, 2.0, nan, -1.0, 7.0, 4.0]], np.float32)
    assert _select_case(J).tolist() == [1, 2, 2, 0, 2, 0, 2]
    assert _select_case(np.array([[nan, 1.0, -2.0]], np.float32)).tolist() == [0, 0, 0]
    rs = np.random.RandomState(5)
    big = rs.standard_normal((9, 300)).astype(np.float32).round(1)          # more than one block; many exact ties
    _select_case(big)


def test_selection_of_a_search_matches_the_oracle():
    name = "delta_mid"
    B, K = lc.CASES[name][3], lc.CASES[name][4]
    got = run_case(name)
    out = select(got["J"], got["z"], got["pred"], got["terms"], K, B)
    best = lc.reference(name)[1]["best"]
    assert out["best"].cpu().tolist() == best.tolist() and (best != 0).any()
    rows = torch.from_numpy(best * B + np.arange(B)).to(DEV)
    assert torch.equal(out["z"], got["z"][rows]) and torch.equal(out["pred"], got["pred"][:, rows])
    assert torch.equal(out["terms"], got["terms"][rows])


# ------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_return_the_documented_codes_and_launch_nothing():
    name = "half1_width1"
    null = ctypes.c_void_p(0)

    def untouched(out):
        assert all(bool((v == 7).all()) for v in out.values())

    for over in (dict(K=0), dict(B=0), dict(ld=1), dict(steps=-1), dict(z0=null), dict(mu=null), dict(lv=null), dict(th=null),
                 dict(tl=null), dict(z_out=null), dict(pred=null), dict(terms=null), dict(J=null), dict(n=null),
                 dict(means=null), dict(logits=null, means=null), dict(C=0), dict(C=4097), dict(homo=null), dict(half=2)):
        untouched(run_case(name, expect=ERR_ARG, **over))
    untouched(run_case(name, expect=ERR_UNSUPPORTED, K=1 << 11, B=1 << 10))
    x = dict(lc.reference(name)[0])
    rs = np.random.RandomState(0)
    x["homo"] = lc.make_head(rs, [1, 513, 1], 0.25)                      # a hidden width past the envelope
    untouched(guided(x, 1, 1, 1, 0.1, 0.0, 2, -1.0, (1.0, 1.0), 0.0, 0.0, expect=ERR_UNSUPPORTED))
    x["homo"] = lc.make_head(rs, [1, 2, 2, 2, 2, 1], 0.25)               # the struct's five Linear layers, said to be six
    hs, keep = head_struct(x["homo"])
    hs.n_linear = 6
    untouched(guided(x, 1, 1, 1, 0.1, 0.0, 2, -1.0, (1.0, 1.0), 0.0, 0.0, expect=ERR_UNSUPPORTED, over=dict(homo=ctypes.byref(hs))))
    J = torch.zeros(4, device=DEV)
    z, pred, terms = torch.zeros(4, 3, device=DEV), torch.zeros(2, 4, device=DEV), torch.zeros(4, 3, device=DEV)
    for over in (dict(K=0), dict(B=0), dict(ld=0), dict(J=null), dict(z=null), dict(pred=null), dict(terms=null),
                 dict(best=null), dict(zb=null), dict(pb=null), dict(tb=null), dict(K=1 << 11, B=1 << 10)):
        out = select(J, z, pred, terms, 2, 2, expect=ERR_ARG, over=over)
        untouched(out)


def test_mixture_pointers_all_null_means_the_standard_normal_whatever_c_says():
    name = "half12_normal"
    got = run_case(name, C=99)
    for k, v in device_run(name).items():
        assert (got[k].cpu().numpy().view(np.int32) == v.view(np.int32)).all(), k


# ------------------------------------------------------------------------------------------ launches
@pytest.mark.parametrize("name", ["half12_normal", "half70_depths"])
def test_one_search_is_one_kernel_launch(name):
    from torch.profiler import profile, ProfilerActivity
    run_case(name)                                                        # warm-up
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run_case(name)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len([n for n in names if "latent_search" in n]) == 1, names
    assert len([n for n in names if "latent_search_guided_k" in n]) == 1, names
