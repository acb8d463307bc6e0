"""GPU: every entry point of csrc/hier_decode.hip called on its own through ``_lib`` (no decode loop) against the fp64
restatement (tests/hier_decode_kernel_oracle.py), rel_err < 1e-4, at the smallest shapes that cross the kernels' loop
boundaries: H 24, 65 (one past a wave), 250, 300 (past one 256-thread stride); clusters of 1, 2, 5, 6 and 30 atoms with 0,
2, 10, 12 and 60 messages; neighbour rows with 0, 1, 3, 9 and 10 live slots in shuffled positions; diterG 1, 2 and 5.  The
resident state is filled with random values first, so a row the call must not touch keeps them: everything outside the
listed rows is compared bit for bit, and the outputs go to buffers wider than needed, filled with a sentinel."""
import ctypes

import numpy as np
import pytest
import torch

import hier_decode_fixtures as HF
import hier_decode_kernel_oracle as HO
from golden_utils import rel_err
from ggpm_amd import _lib
from ggpm_amd import functional as F_
from ggpm_amd import hier_decode as HD

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
BAR = 1e-4
SENTINEL = -777.25
CLUSTERS = (2, 5, 6, 30, 1)         # atoms; a two-atom cluster has 2 messages, a ring of n has 2n, a single atom none
LIVE = (0, 1, 3, 9, 10)
B, N, E, NA, EA, L = 8, 40, 80, 64, 200, 16
SHAPES = [("GRU", 24, 1), ("LSTM", 24, 2), ("GRU", 65, 5), ("LSTM", 65, 1), ("LSTM", 250, 2), ("GRU", 300, 2)]


def _row(rs, width, cnt, pool):
    row = np.zeros(width, np.int64)
    row[rs.permutation(width)[:cnt]] = rs.choice(pool, size=cnt, replace=False)
    return row


def _atom_case(seed, H):
    """the atom tables, a random resident state, and one call's lists.  A listed message's neighbours are drawn half
    from its own cluster's listed messages (so that Jacobi and Gauss-Seidel differ), half from unlisted ones."""
    rs = np.random.RandomState(seed)
    t = {"fnode": rs.standard_normal((NA, 38)).astype(np.float32), "fmess": rs.standard_normal((EA, 62)).astype(np.float32),
         "agraph": np.zeros((EA, 10), np.int64), "bgraph": np.zeros((EA, 10), np.int64)}
    t["h"] = (0.5 * rs.standard_normal((EA, H))).astype(np.float32)
    t["c"] = (0.5 * rs.standard_normal((EA, H))).astype(np.float32)
    t["h"][0] = t["c"][0] = 0
    n_mess = [0 if n == 1 else 2 if n == 2 else 2 * n for n in CLUSTERS]
    ids = rs.permutation(np.arange(1, EA))
    listed, old = ids[:sum(n_mess)], ids[sum(n_mess):]
    atoms = rs.permutation(np.arange(1, NA))[:sum(CLUSTERS)]
    q = 0
    for ci, m in enumerate(n_mess):
        own = listed[q:q + m]
        for j, e in enumerate(own):
            cnt = LIVE[(ci + j) % len(LIVE)]
            others = np.setdiff1d(own, [e])
            k_own = min(len(others), (cnt + 1) // 2)
            pick = np.concatenate([rs.choice(others, k_own, replace=False), rs.choice(old, cnt - k_own, replace=False)])
            t["bgraph"][e, rs.permutation(10)[:cnt]] = pick
        q += m
    for e in old:
        t["bgraph"][e] = _row(rs, 10, rs.randint(0, 11), ids)
    for j, a in enumerate(atoms):
        t["agraph"][a] = _row(rs, 10, LIVE[j % len(LIVE)], ids)
    t["edges"], t["atoms"] = rs.permutation(listed), atoms
    return t


class Harness:
    """the resident state of one decode (HipBackend as the allocator) filled from host arrays; the calls go through
    ``_lib`` directly"""

    def __init__(self, rnn, H, dG, dT=2, seed=3):
        self.rnn, self.H = rnn, H
        self.dec = HF.hier_decoder(rnn, H, L, 20, 60, dT, dG, seed, 0.0).to(DEV)
        rs = np.random.RandomState(seed)
        self.z = [rs.standard_normal((B, L)).astype(np.float32) for _ in range(3)]
        self.be = HD.HipBackend(self.dec, tuple(torch.from_numpy(v).to(DEV) for v in self.z), B, N, E, NA, EA, 5)
        self.p = HO.f64({k: v.detach().cpu().numpy() for k, v in self.dec.state_dict().items()})
        self.lib = _lib.load()

    def put(self, name, value):
        t = getattr(self.be, name) if isinstance(name, str) else name
        t.copy_(torch.as_tensor(np.asarray(value)).to(t.dtype))

    def get(self, name):
        t = getattr(self.be, name) if isinstance(name, str) else name
        return t.cpu().numpy()

    def upload(self, parts):
        flat = []
        for x in parts:
            a = np.asarray(x)
            flat.append((a.astype(np.float32).view(np.int32) if a.dtype.kind == "f" else a.astype(np.int32)).reshape(-1))
        offs = np.cumsum([0] + [p.size for p in flat]).tolist()
        return torch.from_numpy(np.concatenate(flat + [np.zeros(1, np.int32)])).to(DEV), offs

    def atom_step(self, t, stamp, via_edits=True):
        be = self.be
        rows_a, rows_e = np.arange(NA), np.arange(EA)
        parts = [np.zeros((0, 4), np.int32), rows_a, t["fnode"], rows_e, t["fmess"], rows_e, t["agraph"], rows_e, t["bgraph"],
                 t["edges"], t["atoms"]]
        buf, offs = self.upload(parts)
        counts = [0, NA, EA, EA, EA, len(t["edges"]), len(t["atoms"])]
        rc = self.lib.ggpm_hier_decode_atom_step(be.dims, be.state_ptrs, be.param_ptrs, HD._ptr(buf),
                                                 (ctypes.c_int * 12)(*(offs[:11] + [0])), (ctypes.c_int * 7)(*counts), stamp,
                                                 F_._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()


@pytest.mark.parametrize("rnn,H,dG", SHAPES)
def test_atom_step(rnn, H, dG):
    hx = Harness(rnn, H, dG)
    t = _atom_case(7 + H, H)
    be = hx.be
    for buf in be.gh:
        hx.put(buf, t["h"])
    if rnn == "LSTM":
        for buf in be.gc:
            hx.put(buf, t["c"])
    anode0 = np.full((NA, H), SENTINEL, np.float32)
    hx.put("anode", anode0)
    hx.put("astamp", np.full(NA, 3))
    # the restatement first: Jacobi, and -- past one iteration -- not what an in-place update gives
    want_h, want_c, want_rows = HO.atom_step(hx.p, rnn, dG, t["h"], t["c"], t["fnode"], t["fmess"], t["agraph"], t["bgraph"],
                                             t["edges"], t["atoms"])
    want_h = want_h.numpy()
    if dG > 1:
        gs = HO.atom_step_gauss_seidel(hx.p, rnn, dG, t["h"], t["c"], t["fmess"], t["bgraph"], t["edges"]).numpy()
        assert rel_err(gs[t["edges"]], want_h[t["edges"]]) > BAR
    hx.atom_step(t, stamp=9)
    # the tables arrived through the edits
    assert np.array_equal(hx.get("a_fnode"), t["fnode"]) and np.array_equal(hx.get("a_fmess"), t["fmess"])
    assert np.array_equal(hx.get("a_agraph"), t["agraph"]) and np.array_equal(hx.get("a_bgraph"), t["bgraph"])
    listed = np.zeros(EA, bool)
    listed[t["edges"]] = True
    for which, (bufs, want, start) in {"h": (be.gh, want_h, t["h"]),
                                        "c": (be.gc, None if want_c is None else want_c.numpy(), t["c"])}.items():
        if want is None:
            continue
        got = [hx.get(b) for b in bufs]
        assert np.array_equal(got[0], got[1]), which            # both buffers agree after the call
        assert np.array_equal(got[0][~listed], start[~listed]), which   # rows that are not listed keep their bits
        e = rel_err(got[0][listed], want[listed])
        print("atom %s %s H=%d dG=%d rel_err %.2e" % (which, rnn, H, dG, e))
        assert e < BAR, (which, e)
    got = hx.get("anode")
    atoms = np.zeros(NA, bool)
    atoms[t["atoms"]] = True
    assert np.array_equal(got[~atoms], anode0[~atoms])
    e = rel_err(got[t["atoms"]], want_rows.numpy())
    print("atom read-out %s H=%d rel_err %.2e" % (rnn, H, e))
    assert e < BAR, e
    stamps = hx.get("astamp")
    assert (stamps[atoms] == 9).all() and (stamps[~atoms] == 3).all()


def _tree_case(seed, H, stamped):
    rs = np.random.RandomState(seed)
    t = {"fnode": np.stack([rs.randint(0, 20, N), rs.randint(0, 60, N)], axis=1),
         "fmess": np.stack([rs.randint(1, N, E), rs.randint(0, 20, E)], axis=1),
         "agraph": np.zeros((N, 12), np.int64), "bgraph": np.zeros((E, 12), np.int64), "cgraph": np.zeros((N, 30), np.int64)}
    for k in ("ih", "ic", "th", "tc"):
        t[k] = (0.5 * rs.standard_normal((E, H))).astype(np.float32)
        t[k][0] = 0
    nodes = rs.permutation(np.arange(1, N))[:7]
    mess = rs.permutation(np.arange(1, E))[:6]
    old = np.setdiff1d(np.arange(1, E), mess)
    for n in range(1, N):
        t["agraph"][n] = _row(rs, 12, rs.randint(0, 13), np.arange(1, E))
    for j, n in enumerate(nodes):
        t["agraph"][n] = _row(rs, 12, (0, 1, 3, 11, 12)[j % 5], old)
        size = (1, 2, 5, 6, 30, 3, 4)[j]
        t["cgraph"][n, :size] = rs.choice(np.arange(1, NA), size, replace=False)     # stamped and stale atoms alike
    for e in range(1, E):
        t["bgraph"][e] = _row(rs, 12, rs.randint(0, 13), np.arange(1, E))
    for j, e in enumerate(mess):
        t["bgraph"][e] = _row(rs, 12, (0, 1, 3, 11, 12, 2)[j], old)
        t["fmess"][e] = (nodes[j % len(nodes)], (0, 19, 7, 3, 0, 12)[j])
    outsider = int(np.setdiff1d(np.arange(1, N), nodes)[0])
    t["fmess"][mess[-1], 0] = outsider                   # a source that is not among the call's nodes: a zero input row
    t["nodes"], t["mess"] = nodes, np.stack([mess, np.array([2, -1, 0, 5, 7, 1])], axis=1)
    anode = (0.5 * rs.standard_normal((NA, H))).astype(np.float32)
    t["anode"], t["astamp"] = anode, np.where(stamped, 9, 4)
    return t


@pytest.mark.parametrize("rnn,H", [("GRU", 24), ("LSTM", 65), ("LSTM", 250), ("GRU", 300)])
def test_tree_step(rnn, H):
    hx = Harness(rnn, H, 1, dT=2)
    be = hx.be
    rs = np.random.RandomState(H)
    stamped = rs.rand(NA) < 0.6
    t = _tree_case(11 + H, H, stamped)
    tabs = [t[k] for k in ("fnode", "fmess", "agraph", "bgraph", "cgraph")]
    # the tables arrive as edits of the second call; the first call (no messages) reads resident ones
    for name, k in (("t_fnode", "fnode"), ("t_agraph", "agraph"), ("t_cgraph", "cgraph")):
        hx.put(name, t[k])
    for name in ("ih", "ic", "th", "tc"):
        if getattr(be, name) is not None:
            hx.put(name, t[name])
    hx.put("anode", t["anode"])
    hx.put("astamp", t["astamp"])
    hx.put("xi", np.full((B, H), SENTINEL))
    hx.put("xc", np.full((B, H), SENTINEL))
    live = t["anode"] * stamped[:, None]
    n = len(t["nodes"])
    ld = H + 5
    node_out = torch.full((B + 2, ld), SENTINEL, device=DEV)
    mess_out = torch.full((B + 2, ld), SENTINEL, device=DEV)
    buf, offs = hx.upload([t["nodes"]])
    rc = hx.lib.ggpm_hier_decode_tree_step(be.dims, be.state_ptrs, be.param_ptrs, None, 0, HD._ptr(buf), n, None, 0, 9,
                                           F_._p(node_out), ld, F_._p(mess_out), ld, F_._stream())
    assert rc == 0, rc
    want = HO.tree_step(hx.p, rnn, 2, tabs, live, t["ih"], t["ic"], t["th"], t["tc"], t["nodes"], [])
    got = node_out.cpu().numpy()
    assert (got[n:] == SENTINEL).all() and (got[:, H:] == SENTINEL).all() and (mess_out.cpu().numpy() == SENTINEL).all()
    for what, g, w in (("tree read-out", got[:n, :H], want["tnode"]), ("inter input", hx.get("xi")[:n], want["xi"]),
                       ("tree input", hx.get("xc")[:n], want["xc"])):
        e = rel_err(g, w.numpy())
        print("%s %s H=%d rel_err %.2e" % (what, rnn, H, e))
        assert e < BAR, (what, e)
    assert (hx.get("xi")[n:] == SENTINEL).all() and (hx.get("xc")[n:] == SENTINEL).all()
    # the second call: the tree's message tables arrive as edits, six new messages on both levels
    quads = [(2, e, s, t["fmess"][e, s]) for e in range(E) for s in range(2)] + \
        [(1, e, s, t["bgraph"][e, s]) for e in range(E) for s in range(12) if t["bgraph"][e, s]]
    buf, offs = hx.upload([np.asarray(quads), t["nodes"], t["mess"]])
    rc = hx.lib.ggpm_hier_decode_tree_step(be.dims, be.state_ptrs, be.param_ptrs, HD._ptr(buf, offs[0]), len(quads),
                                           HD._ptr(buf, offs[1]), n, HD._ptr(buf, offs[2]), len(t["mess"]), 9, None, 0,
                                           F_._p(mess_out), ld, F_._stream())
    assert rc == 0, rc
    assert np.array_equal(hx.get("t_fmess"), t["fmess"]) and np.array_equal(hx.get("t_bgraph"), t["bgraph"])
    want = HO.tree_step(hx.p, rnn, 2, tabs, live, t["ih"], t["ic"], t["th"], t["tc"], t["nodes"], t["mess"][:, 0])
    rows = np.zeros(E, bool)
    rows[t["mess"][:, 0]] = True
    for name in ("ih", "ic", "th", "tc"):
        if want[name] is None:
            continue
        g = hx.get(name)
        assert np.array_equal(g[~rows], t[name][~rows]), name
        e = rel_err(g[rows], want[name].numpy()[rows])
        print("%s %s H=%d rel_err %.2e" % (name, rnn, H, e))
        assert e < BAR, (name, e)
    got = mess_out.cpu().numpy()
    used = t["mess"][t["mess"][:, 1] >= 0]
    e = rel_err(got[used[:, 1], :H], want["th"].numpy()[used[:, 0]])
    assert e < BAR, e
    rest = np.setdiff1d(np.arange(B + 2), used[:, 1])
    assert (got[rest] == SENTINEL).all() and (got[:, H:] == SENTINEL).all()


def _assm_case(hx, seed):
    """two predictions: five candidates of one atom, six of two; one atom's read-out row is stale (reads as zero)"""
    rs = np.random.RandomState(seed)
    anode = rs.standard_normal((NA, hx.H)).astype(np.float32)
    stamped = np.ones(NA, bool)
    atoms1 = rs.choice(np.arange(1, NA), 5, replace=False)
    atoms2 = rs.choice(np.arange(1, NA), 12, replace=False).reshape(6, 2)
    stamped[atoms2[3, 1]] = False
    meta = [(5, 1, 4, 2, 3, 1, 2), (6, 2, 19, 7, 9, 2, 8)]
    ids = [0, 41, 17, 59, 0]
    atoms = np.concatenate([[0, 0], atoms1, [0], atoms2.reshape(-1), [0]])
    live = anode * stamped[:, None]
    want = np.full(17, np.nan)
    want[3:8] = HO.assm_score(hx.p, live, atoms1.reshape(5, 1), [41], 4, hx.z[2][2]).numpy()
    want[9:15] = HO.assm_score(hx.p, live, atoms2, [17, 59], 19, hx.z[2][7]).numpy()
    return anode, stamped, meta, ids, atoms, want


@pytest.mark.parametrize("rnn,H", [("GRU", 24), ("GRU", 65), ("LSTM", 250), ("GRU", 300)])
def test_assm_score(rnn, H):
    hx = Harness(rnn, H, 1)
    be = hx.be
    anode, stamped, meta, ids, atoms, want = _assm_case(hx, 5 + H)
    for lo, hi in ((3, 8), (9, 15)):        # the restatement's scores are far enough apart to be told apart at the bar
        s = np.sort(want[lo:hi])
        assert np.diff(s).min() >= 1e-3, np.diff(s).min()
    hx.put("anode", anode)
    hx.put("astamp", np.where(stamped, 6, 5))
    buf, offs = hx.upload([np.asarray(meta), ids, atoms])
    score = torch.full((17,), SENTINEL, device=DEV)
    l1, wa = hx.dec.matchNN[0], hx.dec.W_assm
    rc = hx.lib.ggpm_hier_decode_assm_score(
        be.dims, be.state_ptrs, F_._p(hx.dec.E_assm[0].weight), HD._ptr(buf, offs[0]), HD._ptr(buf, offs[1]),
        HD._ptr(buf, offs[2]), 2, 15, len(ids), len(atoms), F_._p(l1.weight), l1.weight.stride(0), F_._p(l1.bias),
        F_._p(wa.weight), F_._p(wa.bias), L, F_._p(be.src_graph), be.src_graph.stride(0), 6, F_._p(score), F_._stream())
    assert rc == 0, rc
    got = score.cpu().numpy()
    assert (got[15:] == SENTINEL).all()
    assert np.isnan(got[:3]).all() and np.isnan(got[8])         # candidates no prediction owns
    for lo, hi in ((3, 8), (9, 15)):
        e = rel_err(got[lo:hi], want[lo:hi])
        print("assm %s H=%d rel_err %.2e" % (rnn, H, e))
        assert e < BAR, e


def test_entry_points_refuse_shapes_outside_the_limits():
    hx = Harness("GRU", 24, 1)
    be = hx.be
    buf, offs = hx.upload([np.arange(1, 4)])
    bad = (ctypes.c_int * 14)(*be.dims)
    bad[1] = 1025
    out = torch.zeros(B, 32, device=DEV)
    args = (be.state_ptrs, be.param_ptrs, None, 0, HD._ptr(buf), 3, None, 0, 1, F_._p(out), 32, F_._p(out), 32, F_._stream())
    assert hx.lib.ggpm_hier_decode_tree_step(bad, *args) != 0
    assert hx.lib.ggpm_hier_decode_tree_step(be.dims, *args[:5], B + 1, *args[6:]) != 0      # more nodes than xi / xc hold
    assert hx.lib.ggpm_hier_decode_tree_step(be.dims, *args) == 0
