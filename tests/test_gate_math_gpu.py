"""GPU: the device gate functions of csrc/common.h, as the level kernels compile them, against fp64.

``ggpm_selftest_gate_math`` (csrc/capi.hip) evaluates ``ggpm_fsigmoid<false>`` (which = 0), ``ggpm_fsigmoid<true>`` (1)
and ``ggpm_sigmoid`` (2) on an array.  The arguments are the sweep of tools/probe/sigmoid_ulp.hip (x = 30 u^3), every
float around the gather sigmoid's worst region (|x| in [16.5, 17], where 1 + e itself rounds) and around its clamp
(|x| in [87.5, 88.5]), the special values, and NaN.  The reference is 1 / (1 + exp(-x)) in numpy fp64; ulp is measured as
the probe does (the unit in the last place of the fp32-rounded exact value).  The bars are the measurements documented
in common.h, rounded up: gather sigmoid worst <= 4 ulp and mean <= 0.5 ulp, libm form worst <= 3 ulp; where the exact
value is below 1e-37 the device flushes denormals and the comparison is absolute (1.2e-38).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = {0: "ggpm_fsigmoid<false>", 1: "ggpm_fsigmoid<true>", 2: "ggpm_sigmoid (libm)"}
FLT_MAX = float(np.finfo(np.float32).max)
SPECIAL = [0.0, 1e-30, 1e-45, 20.0, 88.0, 100.0, 1e4, 1e30, FLT_MAX, float("inf")]
# quiet NaN in both signs, quiet NaN with a payload in both signs, a signalling NaN
NAN_BITS = [0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC12345, 0x7FA00001]


def _every_float(lo, hi):
    """every fp32 value in [lo, hi] (0 < lo < hi), and the mirror image"""
    a, b = (int(np.array([v], dtype=np.float32).view(np.uint32)[0]) for v in (lo, hi))
    pos = np.arange(a, b + 1, dtype=np.uint32).view(np.float32)
    assert pos[0] == np.float32(lo) and pos[-1] == np.float32(hi)
    return np.concatenate([pos, -pos])


def _arguments():
    n0 = 1 << 20
    u = 2.0 * (np.arange(n0, dtype=np.float64) + 0.5) / n0 - 1.0
    sweep = (30.0 * u * u * u).astype(np.float32)
    sp = np.array(SPECIAL, dtype=np.float64).astype(np.float32)          # (1e-45 rounds to the smallest denormal)
    nan = np.array(NAN_BITS, dtype=np.uint32).view(np.float32)
    return np.concatenate([sweep, _every_float(16.5, 17.0), _every_float(87.5, 88.5), sp, -sp, nan])


@pytest.fixture(scope="module")
def table():
    """-> (x fp32, the fp64 sigmoid of every non-NaN x, {which: device result}); computed once, read by every test"""
    from ggpm_amd import _lib
    from ggpm_amd import functional as F_
    x = _arguments()
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x).to(dev)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))       # NaN payloads arrive as sent
    got = {}
    for which in NAMES:
        out = torch.full_like(xd, -7.0)
        _lib.check(_lib.load().ggpm_selftest_gate_math(which, F_._p(xd), xd.numel(), F_._p(out), F_._stream()), "selftest")
        got[which] = out.cpu().numpy()
    with np.errstate(over="ignore"):
        want = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    for a in (x, want, *got.values()):
        a.setflags(write=False)
    return x, want, got


def _ulp_errors(got, want):
    """|got - want| in units of the last place of float(want): tools/probe/sigmoid_ulp.hip's ulp_err"""
    _, e = np.frexp(want.astype(np.float32))
    return np.abs(got.astype(np.float64) - want) / np.ldexp(1.0, e.astype(np.int64) - 24)


def _measure(which, table):
    x, want, got = table
    g = got[which]
    m = ~np.isnan(x) & (want >= 1e-37)
    assert not np.isnan(g[m]).any(), x[m][np.isnan(g[m])][:8]
    err = _ulp_errors(g[m], want[m])
    i = int(err.argmax())
    worst, mean, share = float(err[i]), float(err.mean()), float((err > 1.0).mean())
    print("gate math %-22s worst %.3f ulp at x = %.9g   mean %.4f ulp   above 1 ulp: %.2f %%   (%d arguments)"
          % (NAMES[which], worst, float(x[m][i]), mean, 100.0 * share, int(m.sum())))
    return worst, mean


@pytest.mark.parametrize("which", [0, 1])
def test_gather_sigmoid_accuracy_against_fp64(which, table):
    """common.h documents mean 0.42 ulp, worst 3.4 ulp for ggpm_fsigmoid_acc: worst <= 4 ulp, mean <= 0.5 ulp"""
    worst, mean = _measure(which, table)
    assert worst <= 4.0
    assert mean <= 0.5


def test_libm_sigmoid_accuracy_against_fp64(table):
    """common.h documents worst 2.5 ulp for expf + IEEE division: worst <= 3 ulp"""
    worst, _ = _measure(2, table)
    assert worst <= 3.0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_range_and_special_values(which, table):
    x, want, got = table
    g = got[which]
    ok = ~np.isnan(x)
    assert not np.isnan(g[ok]).any(), x[ok][np.isnan(g[ok])][:8]
    assert ((g[ok] >= 0.0) & (g[ok] <= 1.0)).all()
    tiny = ok & (want < 1e-37)               # flushed denormals: absolute
    assert tiny.any() and (np.abs(g[tiny].astype(np.float64) - want[tiny]) <= 1.2e-38).all()
    hi = ok & (x >= 20.0)
    assert np.isposinf(x[hi]).any() and (g[hi] == np.float32(1.0)).all()
    lo = ok & (x <= -88.0)
    assert np.isneginf(x[lo]).any() and ((g[lo] >= 0.0) & (g[lo] <= 1.2e-38)).all()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_nan_gives_nan(which, table):
    """A NaN gate argument must reach the state: a clamp that answers NaN with a bound (v_med3_f32 returns the smallest
    operand) hides a NaN weight from every isfinite check downstream."""
    x, _, got = table
    nan = np.isnan(x)
    assert int(nan.sum()) == len(NAN_BITS)
    assert np.isnan(got[which][nan]).all(), got[which][nan]
