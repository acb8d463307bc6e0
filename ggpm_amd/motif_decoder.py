"""MotifDecoder -- the tree-only decoder, reference ggpm/decoder.py:475-1095: the teacher-forced training forward
(``sum_forward``; ``mean_forward`` is called nowhere in the reference) and the greedy ``decode`` (ggpm_amd.motif_decode,
which assembles molecules through a graph batch the caller supplies).

Same constructor, sub-module names and ``state_dict`` keys as the reference (``hmpn.*`` -- an ``IncEncoder`` --,
``topoNN``, ``clsNN``, ``iclsNN``, ``matchNN``, ``W_assm``, ``W_root`` when latent != hidden, the aliases ``rnn_cell`` and
``E_assm``), same ``forward(mols, src_mol_vecs, graphs, tensors, orders) -> (loss, cls_acc, icls_acc, topo_acc, assm_acc)``.

The loop's bookkeeping is the hierarchical decoder's minus its atom level, so :class:`ggpm_amd.decoder.DecodeSchedule`
derives it (its atom plan is simply not used).  Device work:
  * the decoder's one level (``IncEncoder``: node input ``E_c[motif]``, message input ``[node of the source visit |
    onehot(pos)]``, the root vectors as B frozen pseudo messages) over the decode-time DAG of ``DecodeSchedule._level_plan``
    as one call per direction into the tree-level driver (csrc/tree_level.hip, embedding-input mode; the default while
    dropout is inactive), or op by op (one sparse-level call, one read-out; dropout active or ``_dev.TREE_DRIVER`` off),
    or the reference's step loop through ``IncEncoder`` (``_dev.DECODER_BATCHED`` off, kept as the checker);
  * topology and cluster heads through ``ScoreHeads`` on the library GEMM, their losses in csrc/losses.hip;
  * ``enum_attach`` + ``get_assm_score`` + the padded cross entropy as ONE launch each way (csrc/motif_assm.hip).
"""
from __future__ import annotations

import contextlib
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _dev
from . import functional as F_
from . import inc_encoder as IE
from .decoder import DecodeSchedule, MAX_POS, _accuracy, _pinned_cls_size, level_states
from .decoder_heads import (ScoreHeads, _i32, _memo, _mlp, bce_rows, bce_with_logits_sum, check_no_dropout,
                            cross_entropy_rows)


class _MotifAssm(torch.autograd.Function):
    """(attachment loss sum, accuracy) of all predictions: ggpm_motif_assm_forward / _backward."""

    @staticmethod
    def forward(ctx, rows, z, W1, b1, Wa, ba, meta, P: int, C: int, n_cand: int):
        from . import _lib
        H, L, B = W1.shape[0], Wa.shape[0], z.shape[0]
        dev = rows.device
        z = z.contiguous()            # (dz is allocated like z and written at row stride z.stride(0))
        rows = rows.contiguous()      # (likewise drows: zeros_like of a column view of a wider buffer is dense)
        act = torch.empty(rows.shape[0], H, dtype=torch.float32, device=dev)
        score = torch.empty(max(n_cand, 1), dtype=torch.float32, device=dev)
        stat = torch.empty(P, 4, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().ggpm_motif_assm_forward(
            F_._p(rows), rows.stride(0), F_._p(meta), P, C, H, L, F_._p(W1), W1.stride(0), F_._p(b1), F_._p(Wa), F_._p(ba),
            F_._p(z), z.stride(0), F_._p(act), F_._p(score), F_._p(stat), F_._p(out), F_._p(counter), F_._stream()),
            "motif_assm_forward")
        ctx.save_for_backward(rows, z, W1, Wa, ba, meta, act, score, stat)
        ctx.dims = (P, C, B)
        acc = out[1]
        ctx.mark_non_differentiable(acc)
        return out[0], acc

    @staticmethod
    def backward(ctx, dloss, _dacc):
        from . import _lib
        rows, z, W1, Wa, ba, meta, act, score, stat = ctx.saved_tensors
        P, C, B = ctx.dims
        H, L = W1.shape[0], Wa.shape[0]
        dloss = dloss.reshape(1).contiguous().float()
        drows = torch.zeros_like(rows)
        dW1 = torch.empty(H, H + MAX_POS, dtype=torch.float32, device=rows.device)
        db1 = torch.empty(H, dtype=torch.float32, device=rows.device)
        dWa, dba = torch.empty_like(Wa), torch.empty_like(ba)
        dz = torch.zeros_like(z)
        _lib.check(_lib.load().ggpm_motif_assm_backward(
            F_._p(dloss), F_._p(rows), rows.stride(0), F_._p(meta), P, C, H, L, B, F_._p(W1), W1.stride(0), F_._p(Wa),
            F_._p(ba), F_._p(z), z.stride(0), F_._p(act), F_._p(score), F_._p(stat), F_._p(drows), F_._p(dW1), F_._p(db1),
            F_._p(dWa), F_._p(dba), F_._p(dz), F_._stream()), "motif_assm_backward")
        return drows, dz, dW1, db1, dWa, dba, None, None, None, None


class _MotifParts(torch.autograd.Function):
    """The four losses of one teacher-forced pass per molecule, parts [B, 4], as ONE node over the heads' scores
    (``molecule_losses`` where autograd records): the loss kernels of ``forward`` with their row losses kept, the attachment
    head's launch and ggpm_mol_loss_parts.  The backward takes ``dparts [B, 4]``: every row's loss gradient is weighed with
    its molecule's entry (ggpm_scale_rows_by_mol, ggpm_motif_assm_backward_weighted)."""

    @staticmethod
    def forward(ctx, topo_scores, cls_scores, icls_scores, rows, z, W1, b1, Wa, ba, spec: dict):
        """``spec``: topo_y fp32, topo_mol / cls_mol int32, clab / ilab int32, mask, B, and with attachment predictions
        meta, pred_mol, P, C, n_cand (``rows`` .. ``ba`` are None without)."""
        from . import _lib
        lib = _lib.load()
        dev, B = topo_scores.device, spec["B"]
        f32 = dict(dtype=torch.float32, device=dev)
        x = topo_scores.contiguous()
        loss = torch.empty(1, **f32)
        topo_rows, dx = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.ggpm_bce_logits(F_._p(x), F_._p(spec["topo_y"]), x.numel(), F_._p(loss), F_._p(dx), F_._p(topo_rows),
                                       F_._stream()), "bce_logits")

        def ce(s, labels, mask=None, mask_row=None):
            M, N = s.shape
            r, d = torch.empty(M, **f32), torch.empty(M, F_._ld(s), **f32)
            if d.shape[1] > N:
                d[:, N:].zero_()
            _lib.check(lib.ggpm_softmax_ce(F_._p(s), F_._ld(s), M, N, F_._p(mask), 0 if mask is None else F_._ld(mask),
                                           F_._p(mask_row), F_._p(labels), F_._p(loss), F_._p(d), d.shape[1], None, F_._p(r),
                                           F_._stream()), "softmax_ce")
            return r, d

        cls_rows, d_c = ce(cls_scores, spec["clab"])
        icls_rows, d_i = ce(icls_scores, spec["ilab"], spec["mask"], spec["clab"])
        assm, P = None, spec.get("P", 0)
        ctx.assm = None
        if P > 0:
            H = W1.shape[0]
            z, rows = z.contiguous(), rows.contiguous()
            act, score = torch.empty(rows.shape[0], H, **f32), torch.empty(max(spec["n_cand"], 1), **f32)
            stat, res = torch.empty(P, 4, **f32), torch.empty(2, **f32)
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.ggpm_motif_assm_forward(
                F_._p(rows), rows.stride(0), F_._p(spec["meta"]), P, spec["C"], H, Wa.shape[0], F_._p(W1), W1.stride(0),
                F_._p(b1), F_._p(Wa), F_._p(ba), F_._p(z), z.stride(0), F_._p(act), F_._p(score), F_._p(stat), F_._p(res),
                F_._p(counter), F_._stream()), "motif_assm_forward")
            assm = (stat.view(-1)[2:], spec["pred_mol"], P, 4)
            ctx.assm = (rows, z, W1, Wa, ba, act, score, stat)
        n_c = cls_rows.numel()
        parts = F_.mol_loss_parts([(topo_rows, spec["topo_mol"], topo_rows.numel()), (cls_rows, spec["cls_mol"], n_c),
                                   (icls_rows, spec["cls_mol"], n_c), assm], B)
        ctx.spec, ctx.grads = spec, (dx, d_c, d_i)
        ctx.widths = (cls_scores.shape[1], icls_scores.shape[1])
        ctx.set_materialize_grads(False)
        return parts

    @staticmethod
    def backward(ctx, dparts):
        from . import _lib
        if ctx.grads is None:       # released below: the loss gradients are scaled in place
            raise F_.second_backward("tree-only decoder losses (per molecule)")
        (dx, d_c, d_i), ctx.grads = ctx.grads, None
        assm, ctx.assm = ctx.assm, None
        if dparts is None:
            return (None,) * 10
        spec = ctx.spec
        B = spec["B"]
        dparts = dparts.to(torch.float32).contiguous()
        F_.scale_rows_by_mol(dx, 1, spec["topo_mol"], dparts[:, 0], B)
        F_.scale_rows_by_mol(d_c, ctx.widths[0], spec["cls_mol"], dparts[:, 1], B)
        F_.scale_rows_by_mol(d_i, ctx.widths[1], spec["cls_mol"], dparts[:, 2], B)
        out = [dx, d_c[:, :ctx.widths[0]], d_i[:, :ctx.widths[1]]] + [None] * 7
        if assm is not None:
            rows, z, W1, Wa, ba, act, score, stat = assm
            H, L, P = W1.shape[0], Wa.shape[0], spec["P"]
            drows, dz = torch.zeros_like(rows), torch.zeros_like(z)
            dW1 = torch.empty(H, H + MAX_POS, dtype=torch.float32, device=rows.device)
            db1 = torch.empty(H, dtype=torch.float32, device=rows.device)
            dWa, dba = torch.empty_like(Wa), torch.empty_like(ba)
            coef = dparts[:, 3]
            _lib.check(_lib.load().ggpm_motif_assm_backward_weighted(
                None, F_._p(coef), max(coef.stride(0), 1), F_._p(rows), rows.stride(0), F_._p(spec["meta"]), P, spec["C"], H, L,
                B, F_._p(W1), W1.stride(0), F_._p(Wa), F_._p(ba), F_._p(z), z.stride(0), F_._p(act), F_._p(score), F_._p(stat),
                F_._p(drows), F_._p(dW1), F_._p(db1), F_._p(dWa), F_._p(dba), F_._p(dz), F_._stream()),
                "motif_assm_backward_weighted")
            out[3:9] = [drows, dz, dW1, db1, dWa, dba]
        return tuple(out)


class AssmPlan:
    """The attachment predictions of one schedule in the reference's order (step major): per prediction one meta row
    {n candidates, k rows per candidate, nth_child, molecule, first candidate, first row}, and the E_assm id of every row
    (``icls * len(cands)``, ggpm/decoder.py:624-626)."""

    def __init__(self, schedule: DecodeSchedule):
        meta, ids, n_cand, n_row = [], [], 0, 0
        for st in schedule.steps:
            for cands, icls, nth, i in st["assm"]:
                n, k = len(cands), len(icls)
                if k not in (1, 2):
                    raise NotImplementedError("MotifDecoder: an attachment of %d atoms (the reference sums pairs only)" % k)
                meta.append((n, k, int(nth), int(i), n_cand, n_row))
                ids.extend(list(icls) * n)
                n_cand += n
                n_row += n * k
        self.P, self.n_cand, self.n_row = len(meta), n_cand, n_row
        self.meta = np.asarray(meta, dtype=np.int32).reshape(-1, 6)
        self.ids = np.asarray(ids, dtype=np.int32)        # (int32: what the gather kernel reads)
        self._dev = None

    def to_device(self, device):
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, torch.as_tensor(self.meta).to(device), torch.as_tensor(self.ids).to(device))
        return self._dev[1], self._dev[2]


def assm_plan(schedule: DecodeSchedule) -> AssmPlan:
    ap = getattr(schedule, "_motif_assm", None)
    if ap is None:
        ap = schedule._motif_assm = AssmPlan(schedule)
    return ap


class MotifDecoder(ScoreHeads):
    """reference ggpm/decoder.py:475-899 (training forward, ``attention=False``)"""

    DECODE_MODULE = "motif_decode"

    def __init__(self, vocab, avocab, rnn_type, embed_size, hidden_size, latent_size, depthT, depthG, dropout,
                 attention=False):
        super().__init__(vocab, embed_size, hidden_size, latent_size, dropout)
        if attention:
            raise NotImplementedError("attention is off in every shipped configuration")
        if embed_size != hidden_size:
            raise ValueError("MotifDecoder: embed_size must equal hidden_size (the reference's IncEncoder and enum_attach "
                             "feed embedding rows where hidden vectors go), got %d and %d" % (embed_size, hidden_size))
        self.avocab = avocab
        self.use_attention = False
        self.hmpn = IE.IncEncoder(vocab, avocab, rnn_type, embed_size, hidden_size, depthT, depthG, dropout)
        self.rnn_cell = self.hmpn.tree_encoder.rnn          # aliases, as the reference registers them
        self.E_assm = self.hmpn.E_i
        self.matchNN = nn.Sequential(nn.Linear(hidden_size + MAX_POS, hidden_size), nn.ReLU())
        if latent_size != hidden_size:
            self.W_root = nn.Linear(latent_size, hidden_size)
        self.graph_batch_factory = None     # decode's graph batch when the call names none (ggpm_amd.motif_decode)

    def schedule_hints(self) -> dict:
        return {}

    # ------------------------------------------------------------------ forward
    def forward(self, mols, src_mol_vecs, graphs, tensors, orders, avg_loss=False, schedule: Optional[DecodeSchedule] = None):
        if avg_loss:
            raise NotImplementedError("MotifDecoder.mean_forward (avg_loss=True) is not part of this build: nothing in the "
                                      "reference calls it")
        tree_tensors, graph_tensors = tensors
        B = len(orders)
        dev = tree_tensors[0].device
        if schedule is None:
            schedule = DecodeSchedule.from_graphs(graphs, tensors, orders, self.vocab)
        D = schedule.to_device(dev)._dev
        src_root_vecs, src_tree_vecs, src_graph_vecs = src_mol_vecs
        init_vecs = self._init_vecs(src_root_vecs)
        if self._batched_schedule(schedule):
            topo_vecs, cls_vecs = self._states_batched(schedule, D, tree_tensors, init_vecs)
        else:
            topo_vecs, cls_vecs = self._states_stepwise(schedule, tree_tensors, graph_tensors, init_vecs)

        topo_scores = self.get_topo_score(src_tree_vecs, D["topo_batch32"], topo_vecs)
        topo_y, clab, ilab = self._labels(D)
        topo_loss = bce_with_logits_sum(topo_scores, topo_y)
        cls_loss, cls_pred, icls_pred = self.cls_losses(src_tree_vecs, D["cls_batch32"], cls_vecs, clab, ilab)
        topo_acc = ((topo_scores.detach() >= 0).long() == D["topo_label"]).float().sum() / D["topo_label"].numel()
        cls_acc, icls_acc = _accuracy(cls_pred, D["cls_clab"]), _accuracy(icls_pred, D["cls_ilab"])
        assm_loss, assm_acc = self.assm_head(schedule, src_graph_vecs)
        loss = (topo_loss + cls_loss + assm_loss) / B
        return loss, cls_acc, icls_acc, topo_acc, assm_acc

    def molecule_losses(self, mols, src_mol_vecs, graphs, tensors, orders, schedule: Optional[DecodeSchedule] = None,
                        max_cls_size: Optional[int] = None, atom=None, out: Optional[torch.Tensor] = None):
        """The per-molecule form of what ``forward`` sums -> [B, 4]: per molecule the sum of its rows' topology BCE,
        motif-class CE, attachment-class CE and attachment CE (``forward``'s loss is their total / B).
        ``max_cls_size``: the number of rows every attachment prediction is padded to (the reference pads to the batch's
        largest cluster x 2 with zero candidates, which score ``b_assm . z``): None takes the batch's own, an int pins it.
        ``atom`` is HierMPNDecoder's argument (this decoder has no atom level: None); ``out``: a contiguous fp32 [B, 4]
        tensor to write.  Forward only unless autograd records -- gradients enabled and a latent vector requiring them:
        then the same values are the output of ONE node over the heads' scores (_MotifParts) whose backward takes
        ``dparts [B, 4]`` (``out`` is not taken then)."""
        from . import _lib
        record = torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in src_mol_vecs)
        if record and out is not None:
            raise ValueError("MotifDecoder.molecule_losses: out= is for the forward-only form (autograd records this call)")
        check_no_dropout(self, "MotifDecoder.molecule_losses runs without dropout: call model.eval() first")
        tree_tensors, graph_tensors = tensors
        B, H, L = len(orders), self.hidden_size, self.latent_size
        dev = tree_tensors[0].device
        if schedule is None:
            schedule = DecodeSchedule.from_graphs(graphs, tensors, orders, self.vocab)
        C = _pinned_cls_size(schedule, max_cls_size)
        src_root_vecs, src_tree_vecs, src_graph_vecs = src_mol_vecs
        with contextlib.nullcontext() if record else torch.no_grad():
            D = schedule.to_device(dev)._dev
            init_vecs = self._init_vecs(src_root_vecs)
            if self._batched_schedule(schedule):
                topo_vecs, cls_vecs = self._states_batched(schedule, D, tree_tensors, init_vecs)
            else:
                topo_vecs, cls_vecs = self._states_stepwise(schedule, tree_tensors, graph_tensors, init_vecs)
            topo_scores = self.get_topo_score(src_tree_vecs, D["topo_batch32"], topo_vecs)
            if record:
                return self._parts_node(schedule, D, C, B, src_tree_vecs, src_graph_vecs, topo_scores, cls_vecs)
            topo_y, clab, ilab = self._labels(D)
            topo_rows = bce_rows(topo_scores, topo_y)
            parts = self._parts(src_tree_vecs, D["cls_batch32"], cls_vecs)
            cls_rows = cross_entropy_rows(_mlp(self.clsNN, *parts), clab)
            vocab = self.vocab
            mask = vocab.mask_on(dev) if hasattr(vocab, "mask_on") else vocab.mask.to(dev)
            icls_rows = cross_entropy_rows(_mlp(self.iclsNN, *parts), ilab, mask=mask, mask_row=clab)
            assm = None
            ap = assm_plan(schedule)
            if ap.P > 0:
                # the head's own launch (csrc/motif_assm.hip): stat[p] = {lse, s0, loss, hit}, so the losses sit 4 floats apart
                meta, ids = ap.to_device(dev)
                rows = IE._embedding_rows(self.E_assm, ids).contiguous()
                z = src_graph_vecs.contiguous()
                l1, wa = self.matchNN[0], self.W_assm
                f32 = dict(dtype=torch.float32, device=dev)
                act, score = torch.empty(rows.shape[0], H, **f32), torch.empty(max(ap.n_cand, 1), **f32)
                stat, res = torch.empty(ap.P, 4, **f32), torch.empty(2, **f32)
                counter = torch.zeros(1, dtype=torch.int32, device=dev)
                _lib.check(_lib.load().ggpm_motif_assm_forward(
                    F_._p(rows), rows.stride(0), F_._p(meta), ap.P, C, H, L, F_._p(l1.weight), l1.weight.stride(0),
                    F_._p(l1.bias), F_._p(wa.weight), F_._p(wa.bias), F_._p(z), z.stride(0), F_._p(act), F_._p(score),
                    F_._p(stat), F_._p(res), F_._p(counter), F_._stream()), "motif_assm_forward")
                pred_mol = _memo(D, "motif_assm_mol32", lambda: meta[:, 3].contiguous())
                assm = (stat.view(-1)[2:], pred_mol, ap.P, 4)
            n_c = cls_rows.numel()
            return F_.mol_loss_parts([(topo_rows, D["topo_batch32"], topo_rows.numel()), (cls_rows, D["cls_batch32"], n_c),
                                      (icls_rows, D["cls_batch32"], n_c), assm], B, out=out)

    def _parts_node(self, schedule, D, C, B, src_tree_vecs, src_graph_vecs, topo_scores, cls_vecs):
        """The differentiable tail of ``molecule_losses``: the class heads' scores, the attachment head's inputs, _MotifParts"""
        dev = topo_scores.device
        topo_y, clab, ilab = self._labels(D)
        parts = self._parts(src_tree_vecs, D["cls_batch32"], cls_vecs)
        cls_scores, icls_scores = _mlp(self.clsNN, *parts), _mlp(self.iclsNN, *parts)
        vocab = self.vocab
        spec = dict(B=B, topo_y=topo_y, topo_mol=_i32(D["topo_batch32"]), cls_mol=_i32(D["cls_batch32"]), clab=clab, ilab=ilab,
                    mask=vocab.mask_on(dev) if hasattr(vocab, "mask_on") else vocab.mask.to(dev))
        ap = assm_plan(schedule)
        if ap.P == 0:
            return _MotifParts.apply(topo_scores, cls_scores, icls_scores, None, None, None, None, None, None, spec)
        meta, ids = ap.to_device(dev)
        spec.update(meta=meta, pred_mol=_memo(D, "motif_assm_mol32", lambda: meta[:, 3].contiguous()), P=ap.P, C=C,
                    n_cand=ap.n_cand)
        l1, wa = self.matchNN[0], self.W_assm
        return _MotifParts.apply(topo_scores, cls_scores, icls_scores, IE._embedding_rows(self.E_assm, ids), src_graph_vecs,
                                 l1.weight, l1.bias, wa.weight, wa.bias, spec)

    def assm_head(self, schedule: DecodeSchedule, src_graph_vecs):
        """(attachment loss sum, accuracy) -- enum_attach, get_assm_score, the cross entropy over max_cls_size rows and
        get_accuracy_sym of ggpm/decoder.py:620-637, 867-892 in one launch (csrc/motif_assm.hip); 0 and 1 without
        attachment predictions, as the reference."""
        ap = assm_plan(schedule)
        if ap.P == 0:
            return 0, 1
        dev = src_graph_vecs.device
        meta, ids = ap.to_device(dev)
        # E_assm rows with the embedding's Dropout applied by torch's module (the masks the tests inject reach the kernel)
        rows = IE._embedding_rows(self.E_assm, ids)
        l1 = self.matchNN[0]
        return _MotifAssm.apply(rows, src_graph_vecs, l1.weight, l1.bias, self.W_assm.weight, self.W_assm.bias, meta, ap.P,
                                schedule.max_cls_size, ap.n_cand)

    def _states_stepwise(self, schedule, tree_tensors, graph_tensors, init_vecs):
        """The reference's loop, step by step (ggpm/decoder.py:790-860): one IncEncoder call per step."""
        dev, H = tree_tensors[0].device, self.hidden_size
        rnn_cell = self.rnn_cell
        htree, tree_tensors = IE.init_decoder_state(rnn_cell, tree_tensors, init_vecs)
        prev = IE.HTuple(vmask=torch.zeros(graph_tensors[0].size(0), dtype=torch.long, device=dev))
        lt = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int64), device=dev)   # noqa: E731
        topo_vecs, cls_vecs = [], [init_vecs]
        for st in schedule.steps:
            subnode, submess = lt(st["subnode"]), lt(st["submess"])
            if submess.numel():
                htree.emask[submess] = 1
            cur = IE.apply_tree_mask(tree_tensors, htree, prev)
            htree = self.hmpn(cur, htree, (subnode, submess))
            topo_vecs.append(htree.node.index_select(0, subnode))
            if len(st["cls_mess"]):
                cls_vecs.append(rnn_cell.get_hidden_state(htree.mess)[:, :H].index_select(0, lt(st["cls_mess"])))
        return torch.cat(topo_vecs, dim=0), torch.cat(cls_vecs, dim=0)

    def _states_batched(self, schedule, D, tree_tensors, init_vecs):
        """Same vectors as ``_states_stepwise`` with the level de-sequentialised (DecodeSchedule._level_plan): every message
        once, over the decode-time DAG.  With dropout inactive the level is ONE driver call per direction
        (csrc/tree_level.hip in its embedding-input mode, ``_dev.TREE_COMPOSITE`` / ``TREE_DRIVER``); otherwise op by op:
        one sparse-level call and ONE read-out over all visits, the Dropout modules applied by torch."""
        hmpn, te, H = self.hmpn, self.hmpn.tree_encoder, self.hidden_size
        P, T = schedule.plan, D["plan"]
        n_inst, depth = P["n_inst"], max(P["chain"], 1)
        from . import tree_decode as TD
        prms = [q for m in (hmpn.E_c, te.W_o, te.rnn) for q in m.parameters()]
        if _dev.TREE_DRIVER and TD.usable((hmpn.E_c[1], te.W_o[2]), prms):
            spec = D.get("motif_level_spec")
            if spec is None:
                B_, E1 = init_vecs.shape[0], P["E1"]
                pre = (D.get("level_structs") or {}).get("tree")
                spec = D["motif_level_spec"] = TD.LevelSpec(
                    T["inst_motif"], T["mess_inst"], T["mess_pos"], T["dag_tree"], T["in_tree"], E1, B_, depth,
                    prebuilt=pre if pre is not None and pre[1].rows == E1 + B_ else None)
            node, hid = TD.tree_level(spec, te.rnn, hmpn.E_c, None, te.W_o, None, init_vecs.contiguous())
            return node[:, :H], torch.cat([init_vecs, hid[:, :H].index_select(0, T["cls_mess"])], dim=0)
        hnode = IE._embedding_rows(hmpn.E_c, T["inst_motif"])                   # E_c's Dropout included
        ld = (H + MAX_POS + 3) // 4 * 4
        src_csr = F_.csr_from_index(T["mess_inst"], ncols=n_inst)
        hmess = F_.tree_message_input(hnode, T["mess_inst"], src_csr, T["mess_pos"], H, MAX_POS, ld)[:, :H + MAX_POS]
        fm = tree_tensors[1]
        h_t = level_states(te.rnn, self.rnn_cell.get_init_state(fm, init_vecs), hmess, T["dag_tree"], depth)
        hid = te.rnn.get_hidden_state(h_t)
        nei = F_.segment_sum(hid, F_.csr_from_padded(T["in_tree"], ncols=hid.shape[0]), H)
        node = F_.linear([hnode, nei], [H, H], te.W_o[0].weight, te.W_o[0].bias, act=F_.ACT_RELU)
        node = te.W_o[2](node)
        cls_vecs = torch.cat([init_vecs, hid[:, :H].index_select(0, T["cls_mess"])], dim=0)
        return node[:, :H], cls_vecs
