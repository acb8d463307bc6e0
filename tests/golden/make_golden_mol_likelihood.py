#!/usr/bin/env python3
"""Golden fixtures for the per-molecule likelihood terms (``log_likelihood`` of the four VAEs), produced by RUNNING THE
REFERENCE:

    python tests/golden/make_golden_mol_likelihood.py          (build container only; needs the reference checkout)

Per case (one per decoder and cell) a synthetic batch goes through the reference's ``MolGraph.tensorize``, its encoder and
``R_mean`` / ``R_var``; for K recorded draws ``eps_k`` the latent ``z_k = mean + exp(lv / 2) * eps_k`` goes through the
reference decoder's teacher-forced ``forward`` on ``(z_k, z_k, z_k)``.  The scores and labels that reach its four loss
modules are captured with forward hooks and the row -> molecule lists where they are handed to ``zip_tensors``; from them
the per-row losses, their per-molecule sums ``parts[K, B, 4]``, ``kl[B]``, ``elbo[B]`` and ``iwae[B]`` are formed in fp64.
Recorded next to them: ``eps``, ``mean``, ``pre_var``, the reference's own batch loss of every pass, and what the test
needs to rebuild the model and the batch.  Written to tests/golden/mol_likelihood/.  Fixtures are DATA; no reference source
text is stored.

The batch seed of a case is the first one from its base seed whose batch has a molecule with attachment predictions and one
without, and two molecules whose largest cluster differs.
"""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_vae as mgv  # noqa: E402

import torch  # noqa: E402

from ggpm_amd import synth  # noqa: E402
from ggpm_amd.params import vae_param_shapes, tied_state_dict, seeded_state_dict  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

OUT = os.path.join(HERE, "mol_likelihood")
K = 3

CASES = [
    # name, decoder, rnn, H, latent, depthT, depthG, diterT, diterG, B, motifs, n_motif, tie, seed
    ("ll_hier_gru_s40", "hier", "GRU", 16, 16, 3, 3, 1, 2, 3, (2, 5), 11, False, 40),
    ("ll_hier_lstm_s41", "hier", "LSTM", 24, 8, 2, 4, 1, 3, 3, (1, 5), 11, True, 41),
    ("ll_motif_gru_s60", "motif", "GRU", 16, 16, 3, 2, 1, 1, 3, (2, 5), 11, False, 60),
    ("ll_motif_lstm_s61", "motif", "LSTM", 24, 8, 2, 2, 2, 1, 3, (1, 5), 11, True, 61),
]


def has_assm(m):
    """Does the molecule make an attachment prediction (a child of a ring motif)?"""
    return any(len(m.clusters[m.parent[i]]) > 2 for i in range(1, m.n_motifs))


def batch_for(seed, B, motifs, n_motif, n_attach):
    for s in [seed] + list(range(seed * 1000, seed * 1000 + 10000)):
        specs = synth.random_batch(s, B, motifs=motifs, n_motif_vocab=n_motif, n_attach_vocab=n_attach)
        assm = [has_assm(m) for m in specs]
        if any(assm) and not all(assm) and len({max(len(c) for c in m.clusters) for m in specs}) > 1:
            return s, specs
    raise RuntimeError("no batch with the asked properties")


def row_losses(kind, scores, labels):
    """fp64 addends of the reference's loss module on the captured (scores, labels)"""
    s = scores.detach().double().numpy()
    y = labels.detach().double().numpy() if kind == "bce" else labels.detach().long().numpy()
    if kind == "bce":
        return np.maximum(s, 0.0) - s * y + np.log1p(np.exp(-np.abs(s)))
    mx = s.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(s - mx).sum(axis=1))
    return lse - s[np.arange(len(s)), y]


def main():
    mg.import_reference()
    import ggpm.decoder as D
    import ggpm.property_vae as PV
    from ggpm.mol_graph import MolGraph
    from ggpm.nnutils import make_cuda
    from ggpm.vocab import common_atom_vocab
    MolGraph.__init__ = mgv.patched_init
    real_zip = D.zip_tensors
    os.makedirs(OUT, exist_ok=True)
    for (name, dec, rnn, H, L, dT, dG, iT, iG, B, motifs, n_motif, tie, seed) in CASES:
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        n_attach = 3 * n_motif
        bseed, specs = batch_for(seed, B, motifs, n_motif, n_attach)
        vocab = IndexPairVocab(n_motif, n_attach)
        mols, graphs, (tree_t, graph_t), orders, homos, lumos = MolGraph.tensorize(
            [[s, 0.0, 0.0] for s in specs], vocab, common_atom_vocab)
        tree_np = [np.asarray(x.numpy()) for x in tree_t[:-1]] + [tree_t[-1]]
        graph_np = [np.asarray(x.numpy()) for x in graph_t[:-1]] + [graph_t[-1]]

        class A:
            pass
        a = A()
        a.vocab, a.atom_vocab, a.rnn_type, a.embed_size, a.hidden_size = vocab, common_atom_vocab, rnn, H, H
        a.depthT, a.depthG, a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = dT, dG, iT, iG, 0.0, L, tie
        out = {}
        if dec == "hier":
            model = PV.HierPropertyVAE(a)
            sd = seeded_state_dict(vae_param_shapes(rnn, H, L, n_motif, n_attach), seed)
            if tie:
                sd = tied_state_dict(sd)
            res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
            assert not res.unexpected_keys, res.unexpected_keys
            assert all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.")) for k in res.missing_keys), res.missing_keys
        else:
            model = PV.PropertyVAE(a)
            shapes = OrderedDict((k, tuple(p.shape)) for k, p in model.named_parameters())
            sd = seeded_state_dict(shapes, seed)
            with torch.no_grad():
                for k, p in model.named_parameters():
                    p.copy_(torch.from_numpy(sd[k]))
            owner = {p.data_ptr(): k for k, p in reversed(list(model.named_parameters()))}
            out["sd_keys"] = np.array(list(model.state_dict().keys()))
            out["sd_src"] = np.array([owner.get(v.data_ptr(), "") for v in model.state_dict().values()])
            out["param_names"] = np.array([k for k, _ in model.named_parameters()])
        model.eval()

        rec = {}

        def zip_spy(tup_list, is_concat=False):
            cols = list(zip(*tup_list))
            b = cols[1]
            rec["mol"].append([int(x) if isinstance(x, int) else int(x.reshape(-1)[0]) for x in b])
            return real_zip(tup_list, is_concat)

        def loss_spy(which, kind):
            def hook(module, inputs, output):
                rec[which] = row_losses(kind, inputs[0], inputs[1])
            return hook

        d = model.decoder
        hooks = [d.topo_loss.register_forward_hook(loss_spy("topo", "bce")),
                 d.cls_loss.register_forward_hook(loss_spy("cls", "ce")),
                 d.icls_loss.register_forward_hook(loss_spy("icls", "ce")),
                 d.assm_loss.register_forward_hook(loss_spy("assm", "ce"))]
        D.zip_tensors = zip_spy
        eps = np.random.RandomState(seed + 29).standard_normal((K, B, L)).astype(np.float32)
        parts = np.zeros((K, B, 4), np.float64)
        ref_loss = np.zeros(K, np.float64)
        with torch.no_grad():
            tensors = make_cuda((tree_np, graph_np))
            root = model.encoder(tensors[0], tensors[1])[0] if dec == "hier" else model.encoder(tensors[0])[0]
            mean, pre_var = model.R_mean(root), model.R_var(root)
            lv = -torch.abs(pre_var)
            for k in range(K):
                rec.clear()
                rec["mol"] = []
                z = mean + torch.exp(lv / 2) * torch.from_numpy(eps[k])
                res = d(mols, (z, z, z), graphs, tensors, orders)
                ref_loss[k] = float(res[0])
                rows_of = [("topo", 0), ("cls", 1), ("icls", 1)] + ([("assm", 2)] if "assm" in rec else [])
                assert len(rec["mol"]) == (3 if "assm" in rec else 2), (name, len(rec["mol"]))
                for t, (which, call) in enumerate(rows_of):
                    mol = np.asarray(rec["mol"][call])
                    assert len(mol) == len(rec[which]), (name, which, len(mol), len(rec[which]))
                    np.add.at(parts[k, :, t], mol, rec[which])
                # the fixture's parts add up to the reference's batch loss x B
                assert abs(parts[k].sum() - ref_loss[k] * B) <= 1e-5 * abs(ref_loss[k] * B), (name, k, parts[k].sum(), ref_loss[k] * B)
        for h in hooks:
            h.remove()
        D.zip_tensors = real_zip
        assert (parts[:, :, 3] > 0).any(axis=0).any() and not (parts[:, :, 3] > 0).any(axis=0).all(), name

        m64, lv64, e64 = mean.double().numpy(), lv.double().numpy(), eps.astype(np.float64)
        kl = -0.5 * (1.0 + lv64 - m64 * m64 - np.exp(lv64)).sum(axis=1)
        z64 = m64[None] + np.exp(lv64 / 2)[None] * e64
        logpq = -0.5 * (z64 ** 2).sum(axis=2) + 0.5 * (e64 ** 2 + lv64[None]).sum(axis=2)
        nll = parts.sum(axis=2)
        w = logpq - nll
        mx = w.max(axis=0)
        iwae = mx + np.log(np.exp(w - mx[None]).sum(axis=0)) - np.log(K)
        elbo = -nll.mean(axis=0) - kl
        # rsample's KL is this one / B
        with torch.no_grad():
            ref_kl = float(PV.HierPropertyVAE.rsample(None, root, model.R_mean, model.R_var, False)[1])
        assert abs(kl.sum() / B - ref_kl) < 1e-5 * kl.sum(), (name, kl.sum() / B, ref_kl)

        out.update(eps=eps, mean=mean.numpy(), pre_var=pre_var.numpy(), parts=parts, kl=kl, elbo=elbo, iwae=iwae,
                   logpq=logpq, ref_loss=ref_loss,
                   ref_max_cls_size=np.int32(max(len(attr) * 2 for _, attr in graphs[0].nodes(data="cluster"))),
                   largest_cluster=np.asarray([max(len(c) for c in m.clusters) for m in specs], np.int32),
                   meta=np.array([H, L, dT, dG, iT, iG, B, n_motif, n_attach, seed, bseed, motifs[0], motifs[1], int(tie), K],
                                 dtype=np.int64),
                   decoder=np.array(dec), rnn=np.array(rnn))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-18s bseed=%d C=%d parts/mol=%s kl=%s elbo=%s iwae=%s -> %.1f KB" % (
            name, bseed, int(out["ref_max_cls_size"]), np.round(parts[0].sum(axis=1), 3).tolist(), np.round(kl, 3).tolist(),
            np.round(elbo, 3).tolist(), np.round(iwae, 3).tolist(), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
