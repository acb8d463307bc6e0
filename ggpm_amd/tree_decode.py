"""One tree-side level of the teacher-forced decoder as ONE autograd node.

``HierMPNDecoder._states_batched`` evaluates the attachment level and the motif level of the decoder each as a chain of
seven coarse ops (reference: ``IncHierMPNEncoder.embed_sub_tree`` + ``IncMPNEncoder.forward``, ggpm/encoder.py:208-245,
165-179, called once per decode step from ggpm/decoder.py:201-222; de-sequentialised over the decode-time DAG, see
``DecodeSchedule._level_plan``):

    finput = E[ids]                               embedding rows of every visit
    hnode  = relu([finput | lower] W^T + b)       W_i / W_c           (``lower``: pooled atom vectors / attachment-level nodes)
    hmess  = [hnode[visit of the message] | onehot(position)]
    h      = sparse_forward(h0, hmess, all real messages, DAG, chain)  (GRU / LSTM message function)
    node   = relu([hnode | sum of the incoming messages revealed] W_o^T + b_o)

Through ``functional.py`` that is seven autograd nodes per level and direction, each with its own argument checks,
allocations and ctypes marshalling -- the full VAE step spends more host time issuing these small ops than the GPU needs
to run them.  ``tree_level`` is the same arithmetic in the same order on the same C entry points (results bit-identical to
the op-by-op path up to the summation order of two fused launches) issued from ONE ``torch.autograd.Function``: the gate
inputs are written straight into the rows they belong to (the op-by-op form scatters them), the parameter gradients
go through the same deferred contractions (``functional._defer_*``).  Used when dropout is inactive and the parameters can be published
(``functional.can_publish``); ``_dev.TREE_COMPOSITE = False`` keeps the op-by-op path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _dev, _lib, fused
from . import functional as F_

MAX_POS = 20


def enabled() -> bool:
    return _dev.TREE_COMPOSITE


class LevelSpec:
    """The index tables of one level of one schedule on one device (built once per schedule, see decoder.py)."""

    def __init__(self, ids, mess_inst, mess_pos, dag, in_table, E1: int, n_extra: int, depth: int, prebuilt=None):
        self.ids, self.mess_inst, self.mess_pos, self.dag, self.in_table = ids, mess_inst, mess_pos, dag, in_table
        self.E1, self.n_extra, self.depth = E1, n_extra, depth
        self.prebuilt = prebuilt          # the four structures below, when the schedule's builder made them (csrc/schedule.hip)
        self.rows = None if prebuilt is not None else torch.arange(1, E1, dtype=torch.long, device=dag.device)

    def structures(self):
        """(frozen mask, predecessor CSR, incoming CSR, message -> visit CSR): part of the schedule's upload, or derived on
        the device and memoised on the index tensors"""
        if self.prebuilt is not None:
            return self.prebuilt
        Etot = self.E1 + self.n_extra
        frozen, pred, _ = F_._sparse_structure(Etot, self.rows, self.dag)
        return (frozen, pred, F_.csr_from_padded(self.in_table, ncols=Etot),
                F_.csr_from_index(self.mess_inst, ncols=self.ids.numel()))


def _composite_forward(ctx, S: LevelSpec, lstm: bool, H: int, He: int, lower, extra, emb, W, b, Wo, bo, rp, infer: bool):
    """The forward of _TreeLevel; ``infer`` (ctx None): its forward-only form, the same launches without stashes."""
    lib = _lib.load()
    P, dev = F_._p, lower.device
    f32 = dict(dtype=torch.float32, device=dev)
    Hp, Hep = F_.padded_hidden(H), F_.padded_hidden(He)
    I = H + MAX_POS
    ldm = (I + 3) // 4 * 4
    E1, depth = S.E1, S.depth
    Etot, ms, n_inst = E1 + S.n_extra, E1 - 1, S.ids.numel()
    cell = F_.cell_for(lstm, rp, I, H)
    G = cell.G
    s = F_._stream()
    frozen, pred, in_csr, src_csr = S.structures()
    # 1-2. visit vectors: relu([E[ids] | lower] W^T + b)
    finput = torch.empty(n_inst, Hep, **f32)
    _lib.check(lib.ggpm_gather_rows(P(emb), F_._ld(emb), P(S.ids), n_inst, He, P(finput), Hep, 0, Hep, s), "gather_rows")
    hnode = torch.empty(n_inst, Hp, **f32)
    ldw = W.stride(0)
    F_.gemm_ksegments(1, n_inst, H, [finput, lower], [Hep, F_._ld(lower)], [W, W[:, He:]], [ldw, ldw], [He, H], hnode, Hp, Hp,
                      bias=b, act=F_.ACT_RELU)
    # 3. message inputs
    hmess = torch.empty(ms, ldm, **f32)
    _lib.check(lib.ggpm_gather_rows(P(hnode), Hp, P(S.mess_inst), ms, H, P(hmess), ldm, 0, 0, s), "gather_rows")
    _lib.check(lib.ggpm_onehot(P(S.mess_pos), ms, MAX_POS, P(hmess), ldm, H, ldm, s), "onehot")
    # 4. hoisted gate inputs, straight into the rows 1 .. E1-1 they belong to (row 0 / the extra rows: zero)
    X = torch.zeros(G, Etot, Hp, **f32)
    cell.project_inputs(hmess, ldm, ms, [X[k][1:] for k in range(G)])
    # 5. start state: zero, the extra (frozen) rows carry `extra`
    hp = torch.zeros(Etot, Hp, **f32)
    if extra is not None:
        hp[E1:, :H] = extra
    cp = torch.zeros(Etot, Hp, **f32) if lstm else None
    save = not infer            # forward-only: the depth loop in two ping-pong slots, no stashes
    Hs, Cs, Qs, St = cell.alloc_state(Etot, depth, save)
    cell.sparse_forward(rows=Etot, depth=depth, h_in=hp, c_in=cp, frozen=frozen, X=X, pred=pred, Hs=Hs, Cs=Cs, Qs=Qs, St=St,
                        wpack=cell.alloc_pack(), save=save, stream=s)
    hid = Hs[depth] if save else Hs[depth & 1]
    # 6. read-out of every visit
    nei = torch.empty(n_inst, Hp, **f32)
    F_._segment_sum_raw(hid, in_csr, H, nei)
    node = torch.empty(n_inst, Hp, **f32)
    ldo = Wo.stride(0)
    F_.gemm_ksegments(1, n_inst, H, [hnode, nei], [Hp, Hp], [Wo, Wo[:, H:]], [ldo, ldo], [H, H], node, Hp, Hp, bias=bo,
                      act=F_.ACT_RELU)
    if infer:
        return node, hid
    ctx.S, ctx.meta = S, (lstm, H, He, extra is not None)
    ctx.save_for_backward(lower, node)          # (an input and an output: through autograd, so that no ctx -> output cycle forms)
    ctx.stash = (finput, hnode, hmess, X[cell.reread], Hs, Cs, Qs, St, nei)
    ctx.prm = (emb, W, b, Wo, bo) + tuple(rp)
    ctx.structs = (frozen, pred, in_csr, src_csr)
    ctx.set_materialize_grads(False)            # (an unused output arrives as None, not as a zero tensor to be added)
    return node, hid


class _TreeLevel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S: LevelSpec, lstm: bool, H: int, He: int, lower, extra, emb, W, b, Wo, bo, *rp):
        return _composite_forward(ctx, S, lstm, H, He, lower, extra, emb, W, b, Wo, bo, rp, infer=False)

    @staticmethod
    def backward(ctx, d_node, d_hid):
        lib = _lib.load()
        S = ctx.S
        lstm, H, He, has_extra = ctx.meta
        if ctx.stash is None:
            raise F_.second_backward("tree-side decoder level")
        finput, hnode, hmess, Xg, Hs, Cs, Qs, St, nei = ctx.stash
        lower, node = ctx.saved_tensors
        ctx.stash = None
        emb, W, b, Wo, bo = ctx.prm[:5]
        rp = ctx.prm[5:]
        frozen, pred, in_csr, src_csr = ctx.structs
        P, dev = F_._p, node.device
        f32 = dict(dtype=torch.float32, device=dev)
        Hp, Hep = F_.padded_hidden(H), F_.padded_hidden(He)
        I = H + MAX_POS
        ldm = hmess.shape[1]
        E1, depth = S.E1, S.depth
        Etot, ms, n_inst = E1 + S.n_extra, E1 - 1, S.ids.numel()
        cell = F_.cell_for(lstm, rp, I, H)
        G = cell.G
        s = F_._stream()
        succ = pred.T
        # ---- read-out: dpre_o -> d(hnode), d(nei) -> d(final state)
        if d_node is None:
            d_node = torch.zeros(n_inst, Hp, **f32)
        d_node = d_node.contiguous()
        dpre_o = torch.empty(n_inst, Hp, **f32)
        _lib.check(lib.ggpm_act_backward(P(d_node), P(node), n_inst, H, Hp, F_.ACT_RELU, 0, P(dpre_o), s), "act_backward")
        d_hnode = torch.empty(n_inst, Hp, **f32)
        d_nei = torch.empty(n_inst, Hp, **f32)
        ldo = Wo.stride(0)
        F_.gemm_grouped(0, 0, n_inst, H, H, [
            dict(A=dpre_o, lda=Hp, B=Wo, ldb=ldo, C=d_hnode, ldc=Hp, n_pad=Hp),
            dict(A=dpre_o, lda=Hp, B=Wo[:, H:], ldb=ldo, C=d_nei, ldc=Hp, n_pad=Hp)])
        if d_hid is not None:
            dHD = d_hid.clone() if d_hid.is_contiguous() else d_hid.contiguous()
            acc = 1
        else:
            dHD = torch.empty(Etot, Hp, **f32)
            acc = 0
        in_T = in_csr.T
        _lib.check(lib.ggpm_segment_sum(P(d_nei), Hp, P(in_T.rowptr), P(in_T.col), Etot, H, P(dHD), Hp, acc, 0 if acc else Hp, s),
                   "segment_sum")
        # ---- the level
        dHin = torch.empty(Etot, Hp, **f32)
        dX = torch.empty(G, Etot, Hp, **f32)
        bufs, hid = cell.dW_buffers()
        dCD = torch.zeros(Etot, Hp, **f32) if lstm else None
        dCin = torch.empty(Etot, Hp, **f32) if lstm else None
        cell.sparse_backward(rows=Etot, depth=depth, frozen=frozen, Xg=Xg, pred=pred, succ=succ, Hs=Hs, Cs=Cs, Qs=Qs, St=St,
                             d_out=dHD, dc_out=dCD, d_in=dHin, dc_in=dCin, dX=dX, dW_hidden=hid,
                             work=cell.backward_workspace(Etot, depth), stream=s)
        dXs = [dX[k][1:E1] for k in range(G)]          # the rows of the real messages: contiguous
        # input halves of the gate weights, gate biases
        dbs = cell.input_half_grads(dXs, hmess, ldm, ms, bufs, interleaved=True)
        for q, g in zip(rp, cell.grads(bufs, hid, dbs)):
            F_._defer_sum(q, g)
        # ---- message inputs -> visit vectors
        dhmess = torch.empty(ms, ldm, **f32)
        F_.gemm_ksegments(0, ms, I, dXs, [Hp] * G, [w for w, _ in cell.gates], [w.stride(0) for w, _ in cell.gates], [H] * G, dhmess,
                          ldm, ldm)
        src_T = src_csr.T
        _lib.check(lib.ggpm_segment_sum(P(dhmess), ldm, P(src_T.rowptr), P(src_T.col), n_inst, H, P(d_hnode), Hp, 1, 0, s),
                   "segment_sum")
        dpre_w = torch.empty(n_inst, Hp, **f32)
        _lib.check(lib.ggpm_act_backward(P(d_hnode), P(hnode), n_inst, H, Hp, F_.ACT_RELU, 0, P(dpre_w), s), "act_backward")
        ldw = W.stride(0)
        d_finput = torch.empty(n_inst, Hep, **f32)
        F_.gemm(0, 0, n_inst, He, H, dpre_w, Hp, W, ldw, d_finput, Hep, Hep)
        d_lower = None
        if ctx.needs_input_grad[4]:
            d_lower = F_._empty_same_layout(lower)
            F_.gemm(0, 0, n_inst, H, H, dpre_w, Hp, W[:, He:], ldw, d_lower, F_._ld(d_lower), lower.shape[1])
        # ---- parameter gradients: one contraction per Linear / one scatter per table at the end of the pass
        F_._defer_linear(W, b, dpre_w, [finput, lower], (He, H))
        F_._defer_linear(Wo, bo, dpre_o, [hnode, nei], (H, H))
        F_._defer_gather(emb, He, d_finput, S.ids)
        d_extra = dHin[E1:, :H] if (has_extra and ctx.needs_input_grad[5]) else None
        return (None, None, None, None, d_lower, d_extra) + (None,) * len(ctx.prm)


class TreeLevelC(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_tree_level"""
    _fields_ = ([(k, ctypes.c_int) for k in ("lstm", "H", "He", "E1", "n_extra", "depth", "n_inst")] +
                [(k, ctypes.c_void_p) for k in ("ids", "mess_inst", "mess_pos", "frozen", "pred_rowptr", "pred_col",
                                                "succ_rowptr", "succ_col", "in_rowptr", "in_col", "inT_rowptr", "inT_col",
                                                "srcT_rowptr", "srcT_col")] +
                [("emb", ctypes.c_void_p), ("ld_emb", ctypes.c_int), ("W", ctypes.c_void_p), ("b", ctypes.c_void_p),
                 ("ld_w", ctypes.c_int), ("Wo", ctypes.c_void_p), ("bo", ctypes.c_void_p), ("ld_wo", ctypes.c_int),
                 ("gate_w", ctypes.c_void_p * 4), ("ld_gate", ctypes.c_int * 4), ("gate_b", ctypes.c_void_p * 4),
                 ("Ur", ctypes.c_void_p), ("bu", ctypes.c_void_p), ("ld_ur", ctypes.c_int),
                 ("lower", ctypes.c_void_p), ("ld_lower", ctypes.c_int), ("extra", ctypes.c_void_p), ("ld_extra", ctypes.c_int)])


class TreeLevelViews(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_tree_level_views"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("finput", "hnode", "hmess", "X", "hp", "cp", "Hs", "Cs", "Qs", "St", "wpack",
                                               "nei", "node")]


class TreeLevelGrads(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_tree_level_grads"""
    _fields_ = [("dgate_w", ctypes.c_void_p * 4), ("ld_dgate", ctypes.c_int * 4), ("dgate_b", ctypes.c_void_p * 4),
                ("dUr", ctypes.c_void_p), ("dbu", ctypes.c_void_p), ("dpre_w", ctypes.c_void_p), ("dpre_o", ctypes.c_void_p),
                ("d_finput", ctypes.c_void_p), ("d_lower", ctypes.c_void_p), ("ld_dlower", ctypes.c_int),
                ("n_pad_dlower", ctypes.c_int), ("dHin", ctypes.c_void_p)]


def _addr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _descriptor(S: LevelSpec, lstm: bool, H: int, He: int, lower, extra, emb, W, b, Wo, bo, rp, backward: bool = True):
    """-> (ggpm_tree_level, the index tables it names).  ``backward`` False: the transposed tables (read by the backward
    only) are neither built nor named."""
    frozen, pred, in_csr, src_csr = S.structures()
    succ, in_T, src_T = (pred.T, in_csr.T, src_csr.T) if backward else (None, None, None)
    n_inst = S.ids.numel()
    cell = F_.cell_for(lstm, rp, H + MAX_POS, H)
    Ur, bu = cell.U_r, cell.b_u
    L = TreeLevelC()
    L.lstm, L.H, L.He, L.E1, L.n_extra, L.depth, L.n_inst = int(lstm), H, He, S.E1, S.n_extra, S.depth, n_inst
    for k, t in (("ids", S.ids), ("mess_inst", S.mess_inst), ("mess_pos", S.mess_pos), ("frozen", frozen),
                 ("pred_rowptr", pred.rowptr), ("pred_col", pred.col), ("in_rowptr", in_csr.rowptr), ("in_col", in_csr.col)):
        setattr(L, k, _addr(t))
    if backward:
        for k, t in (("succ_rowptr", succ.rowptr), ("succ_col", succ.col), ("inT_rowptr", in_T.rowptr),
                     ("inT_col", in_T.col), ("srcT_rowptr", src_T.rowptr), ("srcT_col", src_T.col)):
            setattr(L, k, _addr(t))
    L.emb, L.ld_emb = _addr(emb), F_._ld(emb)
    L.W, L.b, L.ld_w = _addr(W), _addr(b), (W.stride(0) if W is not None else 0)   # (W None: embedding-input mode)
    L.Wo, L.bo, L.ld_wo = _addr(Wo), _addr(bo), Wo.stride(0)
    for k, (w, bb) in enumerate(cell.gates):
        L.gate_w[k], L.ld_gate[k], L.gate_b[k] = _addr(w), w.stride(0), _addr(bb)
    L.Ur, L.bu, L.ld_ur = _addr(Ur), _addr(bu), (Ur.stride(0) if Ur is not None else 0)
    L.lower, L.ld_lower = _addr(lower), (F_._ld(lower) if lower is not None else 0)
    L.extra, L.ld_extra = _addr(extra), (F_._ld(extra) if extra is not None else 0)
    return L, (frozen, pred, succ, in_csr, in_T, src_csr, src_T)


def _tree_level_infer(S: LevelSpec, lstm: bool, H: int, He: int, lower, extra, emb, W, b, Wo, bo, *rp):
    """The forward-only form of _TreeLevelNative (ggpm_tree_level_infer): the same (node, hidden state), bit for bit, with
    no stashes and no transposed tables; the hidden state is a view of the arena, which it keeps alive."""
    lib = _lib.load()
    dev = emb.device
    Hp = F_.padded_hidden(H)
    detach = lambda t: None if t is None else t.detach()
    L, _tables = _descriptor(S, lstm, H, He, detach(lower), detach(extra), emb.detach(), detach(W), detach(b), Wo.detach(),
                            bo.detach(), [detach(t) for t in rp], backward=False)
    n_arena = int(lib.ggpm_tree_level_infer_floats(ctypes.byref(L)))
    arena = torch.empty(n_arena, dtype=torch.float32, device=dev)
    V = TreeLevelViews()
    _lib.check(lib.ggpm_tree_level_infer(ctypes.byref(L), F_._p(arena), n_arena, ctypes.byref(V), F_._stream()),
               "tree_level_infer")
    base, Etot, n_inst = arena.data_ptr(), S.E1 + S.n_extra, S.ids.numel()
    node_off, hs_off = (V.node - base) // 4, (V.Hs - base) // 4 + (S.depth & 1) * Etot * Hp
    return arena[node_off:node_off + n_inst * Hp].view(n_inst, Hp), arena[hs_off:hs_off + Etot * Hp].view(Etot, Hp)


class _TreeLevelNative(torch.autograd.Function):
    """``_TreeLevel`` with each direction as ONE call into csrc/tree_level.hip (ggpm_tree_level_forward / _backward): the same
    launches in the same order (bit-identical results), no per-launch ctypes marshalling and two allocations per direction."""

    @staticmethod
    def forward(ctx, S: LevelSpec, lstm: bool, H: int, He: int, lower, extra, emb, W, b, Wo, bo, *rp):
        lib = _lib.load()
        dev = emb.device
        Hp = F_.padded_hidden(H)
        n_inst, Etot = S.ids.numel(), S.E1 + S.n_extra
        L, tables = _descriptor(S, lstm, H, He, lower, extra, emb, W, b, Wo, bo, rp)
        n_saved = int(lib.ggpm_tree_level_saved_floats(ctypes.byref(L)))
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev)
        V = TreeLevelViews()
        _lib.check(lib.ggpm_tree_level_forward(ctypes.byref(L), F_._p(saved), n_saved, ctypes.byref(V), F_._stream()),
                   "tree_level_forward")
        base = saved.data_ptr()

        def view(addr, rows, cols):
            off = (addr - base) // 4
            return saved[off:off + rows * cols].view(rows, cols)

        Hep = F_.padded_hidden(He)
        node = view(V.node, n_inst, Hp)
        hid = view(V.Hs, (S.depth + 1) * Etot, Hp)[S.depth * Etot:]
        ctx.S, ctx.meta = S, (lstm, H, He, extra is not None)
        ctx.save_for_backward(lower, saved)
        ctx.keep = (L, V, extra, tables)      # (the tables the descriptor names)
        ctx.views = (view(V.finput, n_inst, Hep), view(V.hnode, n_inst, Hp), view(V.nei, n_inst, Hp))
        ctx.prm = (emb, W, b, Wo, bo) + tuple(rp)
        ctx.set_materialize_grads(False)
        return node, hid

    @staticmethod
    def backward(ctx, d_node, d_hid):
        lib = _lib.load()
        S = ctx.S
        lstm, H, He, has_extra = ctx.meta
        lower, saved = ctx.saved_tensors
        if ctx.keep is None:
            raise F_.second_backward("tree-side decoder level")
        L, V, extra, _tables = ctx.keep
        finput, hnode, nei = ctx.views
        emb, W, b, Wo, bo = ctx.prm[:5]
        rp = ctx.prm[5:]
        dev = saved.device
        f32 = dict(dtype=torch.float32, device=dev)
        Hp, Hep = F_.padded_hidden(H), F_.padded_hidden(He)
        n_inst, Etot, E1 = S.ids.numel(), S.E1 + S.n_extra, S.E1
        cell = F_.cell_for(lstm, rp, H + MAX_POS, H)
        dgw = [torch.empty(w.shape, **f32) for w, _ in cell.gates]
        dgb = [torch.empty(H, **f32) if bb is not None else None for _, bb in cell.gates]
        dUr = torch.empty(H, H, **f32) if not lstm else None
        dbu = torch.empty(H, **f32) if not lstm else None
        rows = torch.empty(2, n_inst, Hp, **f32)
        dpre_w, dpre_o = rows[0], rows[1]
        d_finput = torch.empty(n_inst, Hep, **f32)
        dHin = torch.empty(Etot, Hp, **f32)
        d_lower = F_._empty_same_layout(lower) if ctx.needs_input_grad[4] else None
        g = TreeLevelGrads()
        for k in range(cell.G):
            g.dgate_w[k], g.ld_dgate[k], g.dgate_b[k] = _addr(dgw[k]), dgw[k].stride(0), _addr(dgb[k])
        g.dUr, g.dbu = _addr(dUr), _addr(dbu)
        g.dpre_w, g.dpre_o, g.d_finput = _addr(dpre_w), _addr(dpre_o), _addr(d_finput)
        g.d_lower = _addr(d_lower)
        g.ld_dlower, g.n_pad_dlower = (F_._ld(d_lower), lower.shape[1]) if d_lower is not None else (0, 0)
        g.dHin = _addr(dHin)
        if d_node is not None:
            d_node = d_node.contiguous()
        if d_hid is not None:
            d_hid = d_hid.contiguous()
        wb = int(lib.ggpm_tree_level_work_bytes(ctypes.byref(L)))
        work = torch.empty((wb + 3) // 4, **f32)
        # the level's parameter gradients on the second stream (csrc/tree_level.hip): what flows on -- d_lower, on the
        # attachment level the input of the atom level's 2.8 ms backward chain -- is then not queued behind ~145 us of
        # contractions per level.  The deferred-gradient queue (functional._DEFERRED) sums them: on that same stream when it is
        # flushed early, on the main stream once it has waited for this one ("early") at the end of the pass.
        side = F_._side_stream(dev) if (F_.side_stream_enabled() and _dev.TREE_WGRADS_ASIDE) else None
        _lib.check(lib.ggpm_tree_level_backward(ctypes.byref(L), ctypes.byref(V), F_._p(d_node), F_._p(d_hid), ctypes.byref(g),
                                                F_._p(work), work.numel() * 4, F_._stream(),
                                                ctypes.c_void_p(side.cuda_stream) if side is not None else None),
                   "tree_level_backward")
        if side is not None:
            for t in (work, saved):        # read there after this node has returned
                t.record_stream(side)
        for q, gr in zip(rp, cell.grads(dgw, (None, dUr, None, dbu), dgb)):
            F_._defer_sum(q, gr)
        if side is not None:
            F_._DEFERRED.written_on(side)  # the end-of-pass flush waits for the second stream before it reads what was queued
        if W is not None:
            F_._defer_linear(W, b, dpre_w, [finput, lower], (He, H))
        F_._defer_linear(Wo, bo, dpre_o, [hnode, nei], (H, H))
        F_._defer_gather(emb, He, d_finput, S.ids)
        d_extra = dHin[E1:, :H] if (has_extra and ctx.needs_input_grad[5]) else None
        ctx.keep = ctx.views = None
        return (None, None, None, None, d_lower, d_extra) + (None,) * len(ctx.prm)


def usable(modules, params) -> bool:
    """Dropout inactive on every module of the level, deferral on, parameters publishable."""
    if not enabled() or not F_.defer_wgrads_enabled():
        return False
    if any(m.training and m.p > 0 for m in modules):
        return False
    return F_.can_publish(*params)


def tree_level(S: LevelSpec, rnn, emb_seq, lin_seq, wo_seq, lower, extra: Optional[torch.Tensor]):
    """-> (node [n_inst, Hp], hidden state [E1 + extra rows, Hp]) of one tree-side decoder level.  ``lin_seq`` and
    ``lower`` None: the embedding-input mode of the tree-only decoder's level (node input E[ids] itself; driver only)."""
    from .rnn import LSTM
    lstm, rp = isinstance(rnn, LSTM), rnn.level_params()
    emb = emb_seq[0].weight
    if lin_seq is None:
        if lower is not None or not _dev.TREE_DRIVER:
            raise ValueError("tree_level: the embedding-input mode takes no lower level and runs through the driver only")
        if not fused.records_grad([t for t in (extra, emb, wo_seq[0].weight, wo_seq[0].bias) + rp if t is not None]):
            return _tree_level_infer(S, lstm, rnn.hidden_size, emb.shape[1], None, extra, emb, None, None,
                                     wo_seq[0].weight, wo_seq[0].bias, *rp)
        return _TreeLevelNative.apply(S, lstm, rnn.hidden_size, emb.shape[1], None, extra, emb, None, None,
                                      wo_seq[0].weight, wo_seq[0].bias, *rp)
    lower = lower if lower.stride(1) == 1 else lower.contiguous()
    if _dev.TREE_DRIVER and not fused.records_grad([t for t in (lower, extra, emb, lin_seq[0].weight, lin_seq[0].bias,
                                                               wo_seq[0].weight, wo_seq[0].bias) + rp if t is not None]):
        return _tree_level_infer(S, lstm, rnn.hidden_size, emb.shape[1], lower, extra, emb, lin_seq[0].weight,
                                 lin_seq[0].bias, wo_seq[0].weight, wo_seq[0].bias, *rp)
    if not _dev.TREE_DRIVER and not fused.records_grad([t for t in (lower, extra, emb, lin_seq[0].weight, lin_seq[0].bias,
                                                                   wo_seq[0].weight, wo_seq[0].bias) + rp if t is not None]):
        dt = lambda t: None if t is None else t.detach()
        return _composite_forward(None, S, lstm, rnn.hidden_size, emb.shape[1], dt(lower), dt(extra), emb.detach(),
                                  lin_seq[0].weight.detach(), lin_seq[0].bias.detach(), wo_seq[0].weight.detach(),
                                  wo_seq[0].bias.detach(), [t.detach() for t in rp], infer=True)
    node_fn = _TreeLevelNative if _dev.TREE_DRIVER else _TreeLevel      # (the Python composite stays as the checker)
    return node_fn.apply(S, lstm, rnn.hidden_size, emb.shape[1], lower, extra, emb, lin_seq[0].weight, lin_seq[0].bias,
                         wo_seq[0].weight, wo_seq[0].bias, *rp)
