"""GPU: every entry point of csrc/motif_decode.hip called on its own through ``_lib`` (no decode loop), against the fp64
restatements of tests/decode_kernel_oracle.py, at the smallest shapes that take each loop of the kernels round more than
once: H past the 64-lane wave (65), not a multiple of 4 (250), past the 256-thread stride (300), two strides and more
than 64 KiB of dynamic LDS (600); vocabularies wider than 256; k = 16; neighbour rows with 0, 1, 3, 11 and 12 live slots.
Output buffers are pre-filled with a sentinel and wider than the rows: pad columns and unlisted rows must keep it.

Float results: ``golden_utils.rel_err`` against fp64 under the project bar TOL = 1e-4 (a dropped stride, a wrong
neighbour slot or weight column is off by percents; fp32 chains of at most 1 200 terms sit near 1e-6 -- DESIGN.md
section 16 lists what was measured).  Each test prints its worst distance."""
import ctypes

import numpy as np
import pytest
import torch

import decode_kernel_oracle as O
from decode_fixtures import TOL
from golden_utils import rel_err
from ggpm_amd import _lib
from ggpm_amd import functional as F_

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
MAX_POS, MAX_NB = O.MAX_POS, O.MAX_NB
SENT = -777.25                      # float sentinel
ISENT = -123456789                  # int32 sentinel
ERR_ARG = 1                         # GGPM_ERR_ARG (include/ggpm_hip.h)
P = F_._p


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def wide(a, ld, fill=0.0, rows=None):
    """``a`` [R, n] in the first columns of a [rows or R, ld] device buffer filled with ``fill``"""
    a = np.asarray(a, np.float32)
    buf = np.full((a.shape[0] if rows is None else rows, ld), fill, np.float32)
    buf[:a.shape[0], :a.shape[1]] = a
    return dev(buf)


def ld_of(H):
    """a leading dimension wider than the row: the next multiple of 4, or 4 more"""
    ld = (H + 3) // 4 * 4
    return ld if ld > H else H + 4


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def host(t):
    return t.detach().cpu().numpy()


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- tree step
class Tree:
    """the resident tables and states of O.tree_state on the device, and the tree-step call as _Decode marshals it"""

    def __init__(self, d, st):
        te = d.hmpn.tree_encoder
        rnn = te.rnn
        self.lstm = hasattr(rnn, "W_f")
        if self.lstm:
            ws = [rnn.W_i[0].weight, rnn.W_i[0].bias, rnn.W_o[0].weight, rnn.W_o[0].bias, rnn.W_f[0].weight,
                  rnn.W_f[0].bias, rnn.W[0].weight, rnn.W[0].bias]
        else:
            ws = [rnn.W_z.weight, rnn.W_z.bias, rnn.W_r.weight, rnn.U_r.weight, rnn.U_r.bias, rnn.W_h.weight, rnn.W_h.bias]
        self.params = [p.detach().contiguous().to(DEV) for p in [d.hmpn.E_c[0].weight, te.W_o[0].weight, te.W_o[0].bias] + ws]
        self.ptrs = (ctypes.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        self.H, self.N, self.E = st["H"], st["N"], st["E"]
        self.lib = _lib.load()
        self.reset(st)

    def reset(self, st):
        self.fnode, self.fmess, self.agraph, self.bgraph = (dev(st[k].astype(np.int32)) for k in
                                                            ("fnode", "fmess", "agraph", "bgraph"))
        self.h = dev(st["h"])
        self.c = dev(st["c"]) if self.lstm else None

    def step(self, depth, edits=None, n_ne=0, n_te=0, nodes=None, node_out=None, mess=None, mess_out=None, H=None,
             ld_node=None, ld_mess=None):
        n_read = 0 if nodes is None else nodes.numel()
        n_mess = 0 if mess is None else mess.shape[0]
        return self.lib.ggpm_motif_decode_tree_step(
            int(self.lstm), self.H if H is None else H, MAX_POS, depth, self.ptrs, P(self.fnode), P(self.fmess),
            P(self.agraph), P(self.bgraph), self.N, self.E, P(self.h), P(self.c), P(edits), n_ne, n_te, P(nodes), n_read,
            P(node_out), (0 if node_out is None else node_out.stride(0)) if ld_node is None else ld_node, P(mess), n_mess,
            P(mess_out), (0 if mess_out is None else mess_out.stride(0)) if ld_mess is None else ld_mess, F_._stream())


def sentinel_rows(n, ld):
    return torch.full((n, ld), SENT, device=DEV)


@pytest.mark.parametrize("H", [24, 65, 250, 300, 600])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
def test_tree_step_against_fp64(rnn, depth, H):
    """read-outs and new messages of one launch each, every neighbour count, against the fp64 oracle; nothing else is
    written; a work item gives the same bits twice in a launch and alone in another"""
    d = O.decoder(rnn, H, 8, 50, 150)
    p = O.f64(d.state_dict())
    st = O.tree_state(100 + H, H)
    t = Tree(d, st)
    ld = ld_of(H)
    n = len(st["nodes"])
    assert sorted(set(st["cnt_nodes"])) == sorted(set(st["cnt_mess"])) == sorted(O.NB_COUNTS) and 12 <= n + 1 <= 16

    # ---- read-outs: the listed nodes, then node 4 of the list (12 live neighbours) once more
    nodes = np.concatenate([st["nodes"], st["nodes"][4:5]]).astype(np.int32)
    node_out = sentinel_rows(n + 3, ld)
    assert t.step(depth, nodes=dev(nodes), node_out=node_out) == 0
    sync()
    got = host(node_out)
    want = np.stack([O.tree_readout(p, st["h"], st["fnode"], st["agraph"], int(v)).numpy() for v in nodes])
    e_node = rel_err(got[:n + 1, :H], want)
    assert np.all(got[:, H:] == SENT) and np.all(got[n + 1:] == SENT)
    assert np.array_equal(bits(t.h), st["h"].view(np.int32))                      # a read-out writes no state
    alone = sentinel_rows(2, ld)
    assert t.step(depth, nodes=dev(nodes[4:5]), node_out=alone) == 0
    sync()
    assert np.array_equal(bits(node_out[4, :H]), bits(node_out[n, :H]))
    assert np.array_equal(bits(node_out[4, :H]), bits(alone[0, :H])) and np.all(host(alone)[1] == SENT)

    # ---- messages: out_row -1 for every second one; item 4 (12 live neighbours) twice, with a row of its own
    spare = int(np.setdiff1d(np.arange(16), st["mess"][:, 1])[0])
    mess = np.concatenate([st["mess"], [[st["mess"][4, 0], spare]]]).astype(np.int32)
    assert mess[4, 1] >= 0 and st["cnt_mess"][4] == MAX_NB and (st["mess"][:, 1] < 0).sum() == n // 2
    mess_out = sentinel_rows(16, ld)
    assert t.step(depth, mess=dev(mess), mess_out=mess_out) == 0
    sync()
    listed = st["mess"][:, 0]
    want_h, want_c = [], []
    for e in listed:
        he, ce = O.tree_message(p, rnn, depth, st["h"], st["c"], st["fnode"], st["fmess"], st["bgraph"], int(e))
        want_h.append(he.numpy())
        want_c.append(None if ce is None else ce.numpy())
    want_h = np.stack(want_h)
    got_h, got_out = host(t.h), host(mess_out)
    e_h = rel_err(got_h[listed], want_h)
    shown = mess[:, 1] >= 0
    e_out = rel_err(got_out[mess[shown, 1], :H], np.concatenate([want_h, want_h[4:5]])[shown])
    assert np.all(got_out[:, H:] == SENT)
    assert np.all(got_out[np.setdiff1d(np.arange(16), mess[shown, 1])] == SENT)        # out_row -1 writes no row
    others = np.setdiff1d(np.arange(st["E"]), listed)
    assert np.array_equal(bits(t.h)[others], st["h"].view(np.int32)[others])
    e_c = 0.0
    if rnn == "LSTM":
        e_c = rel_err(host(t.c)[listed], np.stack(want_c))
        assert np.array_equal(bits(t.c)[others], st["c"].view(np.int32)[others])
    for k, tab in (("fnode", t.fnode), ("fmess", t.fmess), ("agraph", t.agraph), ("bgraph", t.bgraph)):
        assert np.array_equal(host(tab), st[k]), k
    first = (bits(mess_out[int(mess[4, 1]), :H]), bits(mess_out[spare, :H]), bits(t.h[int(listed[4])]))
    t.reset(st)                                                                 # a fresh copy of the state
    alone = sentinel_rows(2, ld)
    assert t.step(depth, mess=dev(np.asarray([[int(listed[4]), 0]], np.int32)), mess_out=alone) == 0
    sync()
    for b in first:
        assert np.array_equal(b, bits(alone[0, :H]))
    assert np.array_equal(first[2], bits(t.h[int(listed[4])]))

    print("tree step %s depth %d H %d: node_out %.2e, mess_out %.2e, h[e] %.2e, c[e] %.2e"
          % (rnn, depth, H, e_node, e_out, e_h, e_c))
    assert e_node < TOL and e_out < TOL and e_h < TOL and e_c < TOL


def test_tree_step_edits():
    """300 node edits and 700 table edits, no work item: the four tables read back equal a numpy application"""
    H, N, E = 24, 320, 400
    rs = np.random.RandomState(7)
    st = O.tree_state(8, H, N=N, E=E, n_work=12)
    t = Tree(O.decoder("GRU", H, 8, 50, 150), st)
    want = {k: st[k].astype(np.int32).copy() for k in ("fnode", "fmess", "agraph", "bgraph")}
    node_edits = np.stack([rs.choice(N, 300, replace=False), rs.randint(0, 50, 300)], axis=1)
    # one edit per (table, row, slot); slot 11 and both fmess columns among them
    slots = [(0, r, s) for r in range(N) for s in range(MAX_NB)] + [(1, r, s) for r in range(E) for s in range(MAX_NB)] + \
        [(2, r, s) for r in range(E) for s in range(2)]
    pick = [slots[i] for i in rs.choice(len(slots), 700, replace=False)]
    pick[:4] = [(0, 5, 11), (1, 6, 11), (2, 7, 0), (2, 7, 1)]
    pick = list(dict.fromkeys(pick))
    tab_edits = np.asarray([(a, r, s, rs.randint(1, E)) for a, r, s in pick], np.int64)
    assert {tuple(v) for v in tab_edits[:, [0, 2]]} >= {(0, 11), (1, 11), (2, 0), (2, 1)} and len(tab_edits) >= 696
    for nd, v in node_edits:
        want["fnode"][nd] = v
    for a, r, s, v in tab_edits:
        want[("agraph", "bgraph", "fmess")[a]][r, s] = v
    edits = dev(np.concatenate([node_edits.reshape(-1), tab_edits.reshape(-1), [0]]).astype(np.int32))
    assert t.step(1, edits=edits, n_ne=len(node_edits), n_te=len(tab_edits)) == 0
    sync()
    for k, tab in (("fnode", t.fnode), ("fmess", t.fmess), ("agraph", t.agraph), ("bgraph", t.bgraph)):
        assert np.array_equal(host(tab), want[k]), k
        assert not np.array_equal(want[k], st[k]), k
    assert np.array_equal(bits(t.h), st["h"].view(np.int32))


# ---------------------------------------------------------------------------------------------- score heads
@pytest.mark.parametrize("case,H,L,n_out,M", [("topo", 65, 20, 1, 37), ("cls", 250, 24, 701, 37),
                                              ("icls", 300, 260, 2100, 37), ("wide", 600, 56, 258, 3)])
def test_mlp_against_fp64(case, H, L, n_out, M):
    n_motif, n_attach = (n_out, 36) if case in ("cls", "wide") else (50, n_out if case == "icls" else 150)
    d = O.decoder("GRU", H, L, n_motif, n_attach)
    seq = {"topo": d.topoNN, "icls": d.iclsNN}.get(case, d.clsNN)
    l1, l2 = seq[0], seq[3]
    assert tuple(l1.weight.shape) == (H, H + L) and tuple(l2.weight.shape) == (n_out, H)
    W1, b1, W2, b2 = (w.detach().contiguous().to(DEV) for w in (l1.weight, l1.bias, l2.weight, l2.bias))
    rs = np.random.RandomState(H + L)
    B = 9
    vec = rs.standard_normal((M, H)).astype(np.float32)
    ctx = rs.standard_normal((B, L)).astype(np.float32)
    bidx = rs.randint(0, B, M).astype(np.int32)             # repeats, out of order
    bidx[:3] = (B - 1, 0, B - 1)
    ldv, ldc, ldh, ldo = ld_of(H) + 4, L + 3, ld_of(H), n_out + 5
    vec_d, ctx_d, bidx_d = wide(vec, ldv, 1e30), wide(ctx, ldc, 1e30), dev(bidx)
    lib = _lib.load()

    def run(row0, m):
        hid, out = sentinel_rows(m + 1, ldh), sentinel_rows(m + 1, ldo)
        rc = lib.ggpm_motif_decode_mlp(
            ctypes.c_void_p(vec_d.data_ptr() + 4 * row0 * ldv), ldv, ctypes.c_void_p(bidx_d.data_ptr() + 4 * row0), P(ctx_d),
            ldc, m, H, L, P(W1), P(b1), P(W2), P(b2), n_out, int(case == "topo"), P(hid), ldh, P(out), ldo, F_._stream())
        assert rc == 0
        sync()
        return hid, out

    hid, out = run(0, M)
    want_hid, want_out = O.mlp(vec, ctx[bidx], *(host(w) for w in (W1, b1, W2, b2)), sigmoid=case == "topo")
    g_hid, g_out = host(hid), host(out)
    assert np.all(g_hid[:, H:] == SENT) and np.all(g_hid[M:] == SENT)
    assert np.all(g_out[:, n_out:] == SENT) and np.all(g_out[M:] == SENT)
    e_hid, e_out = rel_err(g_hid[:M, :H], want_hid.numpy()), rel_err(g_out[:M, :n_out], want_out.numpy())
    for r in sorted({0, M // 2, M - 1}):                    # a row computed alone: the same bits
        h1, o1 = run(r, 1)
        assert np.array_equal(bits(h1[0, :H]), bits(hid[r, :H])) and np.array_equal(bits(o1[0, :n_out]), bits(out[r, :n_out]))
    print("mlp %s H %d L %d n_out %d: hid %.2e, out %.2e" % (case, H, L, n_out, e_hid, e_out))
    assert e_hid < TOL and e_out < TOL


# ---------------------------------------------------------------------------------------------- hier_topk
def run_topk(cls, icls, owner, k, root):
    """the kernel on [M, n] rows held in wider buffers whose pad columns would win every selection if they were read ->
    (scores fp32 [M, k], motifs, attachments)"""
    M, n_cls, n_icls = cls.shape[0], cls.shape[1], icls.shape[1]
    cls_d, icls_d = wide(cls, n_cls + 3, 1e30), wide(icls, n_icls + 5, 1e30)
    owner_d = dev(np.asarray(owner, np.int32))
    out = torch.full((M + 1, 3 * k), ISENT, dtype=torch.int32, device=DEV)
    rc = _lib.load().ggpm_hier_topk(P(cls_d), n_cls + 3, n_cls, P(icls_d), n_icls + 5, n_icls, P(owner_d), M, k, int(root),
                                    P(out), F_._stream())
    assert rc == 0
    sync()
    o = host(out)
    assert np.all(o[M] == ISENT)
    return o[:M, :k].copy().view(np.float32), o[:M, k:2 * k], o[:M, 2 * k:]


def same_scores(got, want):
    """decode_fixtures.assert_same's rule for floats: within 1e-4, relative above 1 -> the worst ratio to that bound"""
    want = np.asarray(want, np.float64)
    ratio = np.abs(np.asarray(got, np.float64) - want) / (TOL * np.maximum(1.0, np.abs(want)))
    return float(ratio.max())


@pytest.mark.parametrize("root", [False, True], ids=["hier", "root"])
@pytest.mark.parametrize("n_cls,n_icls,k,cap,seed", O.TOPK_CASES)
def test_topk_against_fp64(n_cls, n_icls, k, cap, seed, root):
    cls, icls, owner = O.topk_inputs(n_cls, n_icls, k, seed, cap=cap)
    ws, wc, wa, gap = (O.root_topk if root else O.hier_topk)(cls, icls, owner, k)
    assert gap >= O.MIN_GAP, "seed %d: the fp64 ranking has a gap of %.2e; replace the seed" % (seed, gap)
    if cap is not None:
        assert np.bincount(owner, minlength=n_cls)[wc].max() < k         # every chosen motif owns fewer than k
    s, c, a = run_topk(cls, icls, owner, k, root)
    assert np.array_equal(c, wc), (c, wc)
    assert np.array_equal(a, wa), (a, wa)
    worst = same_scores(s, ws)
    print("topk %s (%d, %d, %d): scores at %.2e of the bound, fp64 gap %.2e" % ("root" if root else "hier", n_cls, n_icls, k,
                                                                             worst, gap))
    assert worst <= 1.0


@pytest.mark.parametrize("name", O.topk_fixture_names())
def test_topk_against_the_recorded_reference(name):
    g = O.TopkGolden(name)
    for root, want, k in ((False, g.hier, g.k), (True, g.root, g.k_root)):
        ws, wc, wa = g.split(want, k)
        s, c, a = run_topk(g.cls, g.icls, g.owner, k, root)
        assert np.array_equal(c, wc) and np.array_equal(a, wa), (name, root)
        assert same_scores(s, ws) <= 1.0


def test_topk_ties_go_to_the_lower_index():
    cls, icls, owner, k, expected = O.tie_case()
    for mode, fn in (("hier", O.hier_topk), ("root", O.root_topk)):
        ws, wc, wa, gap = fn(cls, icls, owner, k, ties=True)
        assert gap >= O.MIN_GAP and (wc[0].tolist(), wa[0].tolist()) == expected[mode]
        s, c, a = run_topk(cls, icls, owner, k, mode == "root")
        assert (c[0].tolist(), a[0].tolist()) == expected[mode], (mode, c, a)
        assert same_scores(s, ws) <= 1.0
        if mode == "hier":
            assert s[0, 0] == s[0, 1] and s[0, 2] == s[0, 3] == s[0, 4]
    # a root motif that owns fewer than k: the masked attachments follow by raw score, equal ones by index
    one = np.eye(300, dtype=np.float32)[3:4]
    ws, wc, wa, _ = O.root_topk(one, icls, owner, 8, ties=True)
    s, c, a = run_topk(one, icls, owner, 8, True)
    assert a[0].tolist() == wa[0].tolist() == [7, 400, 401, 402, 3, 67, 259, 4] and c[0].tolist() == [3] * 8
    assert same_scores(s, ws) <= 1.0


# ---------------------------------------------------------------------------------------------- attachment scores
@pytest.mark.parametrize("H,L", [(65, 20), (250, 24), (300, 260), (600, 56)])
def test_assm_score_against_fp64(H, L):
    n_ids, B = 150, 5
    d = O.decoder("GRU", H, L, 50, n_ids)
    p = O.f64(d.state_dict())
    l1, wa = d.matchNN[0], d.W_assm
    W1, b1, Wa, ba, E = (w.detach().contiguous().to(DEV) for w in (l1.weight, l1.bias, wa.weight, wa.bias,
                                                                   d.E_assm[0].weight))
    ldw = W1.stride(0)
    assert ldw == H + MAX_POS and tuple(E.shape) == (n_ids, H)
    rs = np.random.RandomState(3 * H + L)
    z = rs.standard_normal((B, L)).astype(np.float32)
    z_d = wide(z, L + 3, 1e30)
    # (n candidates, k, nth, molecule): every n, both k, both ends of the onehot, molecules out of order
    preds = [(1, 1, 0, 4), (2, 2, 19, 0), (6, 1, 19, 3), (300, 2, 0, 1), (2, 1, 7, 4), (6, 2, 19, 2), (300, 1, 19, 0),
             (1, 2, 0, 3), (6, 2, 3, 1)]

    preds = [pr + ([int(v) for v in rs.randint(0, n_ids, pr[1])],) for pr in preds]

    def launch(items):
        meta, ids, coff = [], [], 2                     # two unlisted scores first, one between any two predictions
        for n, k, nth, b, own in items:
            meta.append((n, k, nth, b, coff, len(ids)))
            ids += own
            coff += n + 1
        score = torch.full((coff + 4,), SENT, device=DEV)
        meta_d, ids_d = dev(np.asarray(meta, np.int32)), dev(np.asarray(ids + [0], np.int32))
        rc = _lib.load().ggpm_motif_decode_assm_score(
            P(E), n_ids, H, L, P(meta_d), P(ids_d), len(meta), P(W1), ldw, P(b1), P(Wa), P(ba), P(z_d), L + 3, P(score),
            F_._stream())
        assert rc == 0
        sync()
        listed = np.zeros(coff + 4, bool)
        for n, _, _, _, off, _ in meta:
            listed[off:off + n] = True
        assert np.all(host(score)[~listed] == SENT)
        return meta, score

    meta, score = launch(preds)
    got, got_one, want_one = host(score), [], []
    for (n, k, nth, b, own), (_, _, _, _, coff, _) in zip(preds, meta):
        want = O.assm_score(p, n, own, nth, z[b]).numpy()
        assert len(want) == n
        assert np.all(got[coff:coff + n] == got[coff])                  # the kernel computes a prediction's score once
        got_one.extend(got[coff:coff + n])                              # ... every candidate against its own fp64 score
        want_one.extend(want)
    err = rel_err(got_one, want_one)
    # two guarded rows (k = 3; nth = ldw - H, one past the onehot) among the others: NaN for them, the rest bit for bit
    bad = [(6, 3, 0, 2, [1, 2, 3]), (2, 1, ldw - H, 1, [5])]
    meta2, score2 = launch(preds[:3] + bad[:1] + preds[3:7] + bad[1:] + preds[7:])
    got2 = host(score2)
    for i in (3, 8):
        assert np.all(np.isnan(got2[meta2[i][4]:meta2[i][4] + meta2[i][0]]))
    kept = [m for i, m in enumerate(meta2) if i not in (3, 8)]
    for (n, _, _, _, coff, _), (n2, _, _, _, coff2, _) in zip(meta, kept):
        assert n == n2 and np.array_equal(bits(score2)[coff2:coff2 + n], bits(score)[coff:coff + n])
    print("assm score H %d L %d: %.2e" % (H, L, err))
    assert err < TOL


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what,k,n_icls,ld_cls", [("k = 17", 17, 40, 20), ("n_icls < k", 5, 4, 20), ("ld_cls < n_cls", 5, 40, 19)])
def test_topk_refuses(what, k, n_icls, ld_cls):
    n_cls, M = 20, 2
    cls, icls = torch.zeros(M, 24, device=DEV), torch.zeros(M, 48, device=DEV)
    owner = torch.zeros(48, dtype=torch.int32, device=DEV)
    out = torch.full((M, 3 * 17), ISENT, dtype=torch.int32, device=DEV)
    rc = _lib.load().ggpm_hier_topk(P(cls), ld_cls, n_cls, P(icls), 48, n_icls, P(owner), M, k, 0, P(out), F_._stream())
    sync()
    assert rc == ERR_ARG, what
    assert np.all(host(out) == ISENT)


@pytest.mark.parametrize("what", ["reads and messages", "ld_node < H", "H = 1025"])
def test_tree_step_refuses(what):
    H = 24
    st = O.tree_state(9, H)
    t = Tree(O.decoder("GRU", H, 8, 50, 150), st)
    nodes, mess = dev(st["nodes"][:2]), dev(st["mess"][:2])
    node_out, mess_out = sentinel_rows(4, 28), sentinel_rows(16, 28)
    if what == "reads and messages":
        rc = t.step(1, nodes=nodes, node_out=node_out, mess=mess, mess_out=mess_out)
    elif what == "ld_node < H":
        rc = t.step(1, nodes=nodes, node_out=node_out, ld_node=H - 1)
    else:
        rc = t.step(1, nodes=nodes, node_out=node_out, H=1025, ld_node=1028)
    sync()
    assert rc == ERR_ARG, what
    assert np.all(host(node_out) == SENT) and np.all(host(mess_out) == SENT)
    assert np.array_equal(bits(t.h), st["h"].view(np.int32))
