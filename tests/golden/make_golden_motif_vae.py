#!/usr/bin/env python3
"""Golden fixtures for the tree-only models 'prop' / 'prop-opt', produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_motif_vae.py          (build container only; needs the reference checkout)

Per case a synthetic batch goes through the reference's ``MolGraph.tensorize`` and then through the reference's own
``PropertyVAE(args)`` or ``PropOptVAE(args)`` step (``perturb_z=False``, dropout 0): ``MotifEncoder``, ``rsample``, the
teacher-forced ``MotifDecoder.sum_forward`` with its ``enum_attach`` and the four losses, then ``backward()``.
Recorded: loss, KL, the metrics, every parameter gradient (full, or probes + statistics for the big ones), the
state_dict key list (with, per key, the parameter it aliases), and the reference's bookkeeping of the decoder loop (the
``subtree`` pair of every step, the ``zip_tensors`` lists and the real-candidate count of every attachment prediction).
Parameters are ``params.seeded_state_dict`` over the reference model's own parameter list.  Written to
tests/golden/motif_vae/.  Fixtures are DATA; no reference source text is stored.
"""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_inc as mgi  # noqa: E402
import make_golden_vae as mgv  # noqa: E402

import torch  # noqa: E402

from ggpm_amd import synth  # noqa: E402
from ggpm_amd.params import seeded_state_dict  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

OUT = os.path.join(HERE, "motif_vae")
BETA = 0.1

CASES = [
    # name, model, rnn, H, latent, depthT, diterT, B, motifs, n_motif, tie, linear_hidden, loss_scaling, seed, full
    ("prop_gru_s60", "prop", "GRU", 16, 16, 3, 1, 3, (2, 5), 11, False, None, False, 60, True),
    ("prop_lstm_s61", "prop", "LSTM", 24, 8, 2, 2, 3, (1, 5), 11, True, None, False, 61, True),
    ("prop_lstm_cfg_s62", "prop", "LSTM", 250, 24, 20, 1, 20, (6, 12), 50, False, None, False, 62, False),
    ("propopt_gru_s63", "prop-opt", "GRU", 16, 8, 3, 1, 3, (2, 5), 11, True, 16, False, 63, True),
    ("propopt_lstm_s64", "prop-opt", "LSTM", 20, 8, 2, 1, 4, (2, 4), 11, True, [8, 8], True, 64, True),
    ("prop_gru_noassm", "prop", "GRU", 16, 12, 2, 1, 3, (2, 4), 11, False, None, False, 65, True),
]


def has_assm(specs):
    """Does the batch make an attachment prediction (a child of a ring motif)?"""
    return any(len(m.clusters[m.parent[i]]) > 2 for m in specs for i in range(1, m.n_motifs))


def batch_for(name, seed, B, motifs, n_motif, n_attach):
    if not name.endswith("noassm"):
        return seed, synth.random_batch(seed, B, motifs=motifs, n_motif_vocab=n_motif, n_attach_vocab=n_attach)
    for s in range(seed * 1000, seed * 1000 + 10000):     # first seed whose batch has no attachment prediction
        specs = synth.random_batch(s, B, motifs=motifs, n_motif_vocab=n_motif, n_attach_vocab=n_attach)
        if not has_assm(specs) and sum(m.n_motifs for m in specs) > B + 1:
            return s, specs
    raise RuntimeError("no batch without attachment predictions")


def main():
    mg.import_reference()
    import ggpm.decoder as D
    import ggpm.property_vae as PV
    from ggpm.mol_graph import MolGraph
    from ggpm.vocab import common_atom_vocab
    MolGraph.__init__ = mgv.patched_init
    real_zip = D.zip_tensors
    os.makedirs(OUT, exist_ok=True)
    for (name, kind, rnn, H, L, dT, iT, B, motifs, n_motif, tie, hidden, scaling, seed, full) in CASES:
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        n_attach = 3 * n_motif
        bseed, specs = batch_for(name, seed, B, motifs, n_motif, n_attach)
        vocab = IndexPairVocab(n_motif, n_attach)
        rs = np.random.RandomState(seed + 17)
        th = (rs.standard_normal(B) * 0.7 - 0.5).astype(np.float32)
        tl = (rs.standard_normal(B) * 0.7 + 0.5).astype(np.float32)
        mols, graphs, (tree_t, graph_t), orders, homos, lumos = MolGraph.tensorize(
            [[s, float(h), float(u)] for s, h, u in zip(specs, th, tl)], vocab, common_atom_vocab)
        tree_np = [np.asarray(x.numpy()) for x in tree_t[:-1]] + [tree_t[-1]]
        graph_np = [np.asarray(x.numpy()) for x in graph_t[:-1]] + [graph_t[-1]]

        class A:
            pass
        a = A()
        a.vocab, a.atom_vocab, a.rnn_type, a.embed_size, a.hidden_size = vocab, common_atom_vocab, rnn, H, H
        a.depthT, a.depthG, a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = dT, 2, iT, 1, 0.0, L, tie
        if kind == "prop-opt":
            a.linear_hidden_size, a.property_optim_step, a.loss_scaling = hidden, 20, scaling
            model = PV.PropOptVAE(a)
        else:
            model = PV.PropertyVAE(a)
        names = [k for k, _ in model.named_parameters()]
        shapes = OrderedDict((k, tuple(p.shape)) for k, p in model.named_parameters() if p.dtype == torch.float32)
        sd = seeded_state_dict(shapes, seed)
        if scaling:
            r2 = np.random.RandomState(seed + 13)
            for k in ("homo_log_var", "lumo_log_var", "recon_log_var"):
                sd["loss_weigh." + k] = (0.5 * r2.standard_normal(1)).astype(np.float64)
        with torch.no_grad():
            for k, p in model.named_parameters():
                p.copy_(torch.from_numpy(sd[k]))
        owner = {p.data_ptr(): k for k, p in reversed(list(model.named_parameters()))}
        sd_keys = list(model.state_dict().keys())
        sd_src = [owner.get(v.data_ptr(), "") for v in model.state_dict().values()]

        rec = {"zip": [], "steps": [], "assm_n": []}

        def zip_spy(tup_list, is_concat=False):
            cols = list(zip(*tup_list))
            rec["zip"].append([list(c) if isinstance(c[0], int) else
                               [t.tolist() if t.dtype == torch.long else tuple(t.shape) for t in c] for c in cols])
            return real_zip(tup_list, is_concat)

        real_enum = model.decoder.enum_attach

        def enum_spy(hgraph, cands, icls, nth_child):
            out = real_enum(hgraph, cands, icls, nth_child)
            rec["assm_n"].append(len(out))
            return out

        def hmpn_spy(module, inputs):
            subtree = inputs[2]
            rec["steps"].append([x.tolist() for x in subtree])

        D.zip_tensors = zip_spy
        model.decoder.enum_attach = enum_spy
        hook = model.decoder.hmpn.register_forward_pre_hook(hmpn_spy)
        out3 = model(mols, graphs, (tree_np, graph_np), orders, homos, lumos, beta=BETA, perturb_z=False)
        hook.remove()
        del model.decoder.enum_attach
        D.zip_tensors = real_zip
        loss, metrics = out3[0], out3[1]
        if kind == "prop-opt":
            assert not out3[2]
        loss.backward()

        out = {"loss": np.asarray(loss.detach().double().numpy()).reshape(()),
               "metric_names": np.array(list(metrics.keys())),
               "metric_values": np.array([float(v) for v in metrics.values()], np.float64),
               "none_grads": np.array(sorted(k for k, p in model.named_parameters() if p.grad is None)),
               "sd_keys": np.array(sd_keys), "sd_src": np.array(sd_src), "param_names": np.array(names),
               "t_homo": th, "t_lumo": tl}
        for k, prm in model.named_parameters():
            if prm.grad is None:
                continue
            g = prm.grad.double().numpy() if prm.dtype == torch.float64 else prm.grad.numpy()
            if full or g.size <= 20000:
                out["grad/" + k] = g
            else:
                out["gprobe/" + k] = g.reshape(-1)[mg.probe_indices(k, g.size, seed)]
                out["gstat/" + k] = np.array([g.sum(dtype=np.float64), np.sqrt((g.astype(np.float64) ** 2).sum()),
                                              np.abs(g).max()])
        for k, v in sd.items():
            if v.dtype == np.float64:
                out["w64/" + k] = v
        for i, col in enumerate(("subnode", "submess")):
            out["ref_" + col], out["ref_" + col + "_off"] = mgi.ragged([s[i] for s in rec["steps"]])
        out["ref_topo_batch"], out["ref_topo_label"] = (np.asarray(rec["zip"][0][1], np.int32),
                                                        np.asarray(rec["zip"][0][2], np.int32))
        out["ref_cls_batch"], out["ref_cls_clab"], out["ref_cls_ilab"] = (np.asarray(c, np.int32) for c in rec["zip"][1][1:4])
        out["ref_assm_batch"] = np.asarray([b[0] for b in rec["zip"][2][1]] if len(rec["zip"]) > 2 else [], np.int32)
        out["ref_assm_n"] = np.asarray(rec["assm_n"], np.int32)
        out["ref_max_cls_size"] = np.int32(max(len(attr) * 2 for _, attr in graphs[0].nodes(data="cluster")))
        for i, k in enumerate(("fnode", "fmess", "agraph", "bgraph", "cgraph")):
            out["tree_" + k] = tree_np[i].astype(np.int32)
        out["tree_scope"] = np.asarray(tree_np[-1], dtype=np.int32)
        for i, k in enumerate(("fnode", "fmess", "agraph", "bgraph")):
            out["graph_" + k] = graph_np[i].astype(np.int32)
        out["graph_scope"] = np.asarray(graph_np[-1], dtype=np.int32)
        out["meta"] = np.array([H, L, dT, iT, B, n_motif, n_attach, seed, bseed, motifs[0], motifs[1], int(tie),
                                int(scaling), int(full)], dtype=np.int64)
        out["kind"], out["rnn"], out["beta"] = np.array(kind), np.array(rnn), np.array(BETA)
        out["linear_hidden"] = np.array([0] if hidden is None else ([hidden] if isinstance(hidden, int) else hidden), np.int64)
        out["linear_hidden_is_int"] = np.array(isinstance(hidden, int))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-18s steps=%d topo=%d cls=%d assm=%d loss=%.6f metrics=%s none=%s -> %.1f KB" % (
            name, len(rec["steps"]), len(rec["zip"][0][1]), len(rec["zip"][1][1]), len(rec["assm_n"]), float(out["loss"]),
            np.round(out["metric_values"], 4).tolist(), out["none_grads"].tolist(), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
