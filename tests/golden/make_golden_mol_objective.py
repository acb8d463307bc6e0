#!/usr/bin/env python3
"""Golden fixtures for ``bound_loss`` (the trainable K-sample ELBO / IWAE objective of the four VAEs), produced by RUNNING
THE REFERENCE:

    python tests/golden/make_golden_mol_objective.py          (build container only; needs the reference checkout)

The four cases, batches and recorded draws (K = 3) are those of make_golden_mol_likelihood.py.  Per case the reference's
encoder, ``R_mean`` / ``R_var`` and -- for each draw -- its decoder's teacher-forced ``forward`` run WITH autograd; the scores
that reach the decoder's four loss modules are captured with forward hooks and stay attached to the graph.  From them the
row losses, their per-molecule sums ``parts[K, B, 4]``, ``kl[B]`` and ``logpq[K, B]`` are formed in torch, then the
objective of one of three variants

    elbo_b03_w : (1/B) sum_i w_i ((1/K) sum_k nll[k, i] + 0.3 kl[i]),          w = [0.5, 2.0, 1.25]
    iwae       : -(1/B) sum_i (logsumexp_k (logpq - nll)[k, i] - log K)
    iwae_w     : the same with the weights w

and ``backward()`` through the reference model.  Recorded per case and variant: the loss and every parameter's gradient from a
fp32 run and from a fp64 run (both stored as float32), the fp64 run's parts / logpq / kl, and what the test needs to rebuild
the model and the batch.  Written to tests/golden/mol_objective/<case>__<variant>.npz.  Fixtures are DATA; no reference
source text is stored.
"""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_vae as mgv  # noqa: E402
import make_golden_mol_likelihood as mll  # noqa: E402

import torch  # noqa: E402

from ggpm_amd.params import vae_param_shapes, tied_state_dict, seeded_state_dict  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402

OUT = os.path.join(HERE, "mol_objective")
K = mll.K
WEIGHTS = [0.5, 2.0, 1.25]
VARIANTS = [("elbo_b03_w", "elbo", 0.3, WEIGHTS), ("iwae", "iwae", 1.0, None), ("iwae_w", "iwae", 1.0, WEIGHTS)]


def row_losses(kind, scores, labels):
    """the addends of the reference's loss module on the captured (scores, labels), attached to the graph"""
    if kind == "bce":
        y = labels.to(scores.dtype)
        return torch.clamp(scores, min=0) - scores * y + torch.log1p(torch.exp(-torch.abs(scores)))
    return torch.logsumexp(scores, dim=1) - scores.gather(1, labels.long().view(-1, 1)).squeeze(1)


def objective(kind, beta, w, parts, logpq, kl):
    B = kl.shape[0]
    w = torch.ones_like(kl) if w is None else torch.as_tensor(w, dtype=kl.dtype)
    nll = parts.sum(dim=2)
    if kind == "elbo":
        return (w * (nll.mean(dim=0) + beta * kl)).sum() / B
    return -(w * (torch.logsumexp(logpq - nll, dim=0) - float(np.log(K)))).sum() / B


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
    worst = {"elbo": 0.0, "iwae": 0.0}
    for (name, dec, rnn, H, L, dT, dG, iT, iG, B, motifs, n_motif, tie, seed) in mll.CASES:
        assert B == len(WEIGHTS)
        n_attach = 3 * n_motif
        bseed, specs = mll.batch_for(seed, B, motifs, n_motif, n_attach)
        vocab = IndexPairVocab(n_motif, n_attach)
        eps = np.random.RandomState(seed + 29).standard_normal((K, B, L)).astype(np.float32)
        runs = {}
        extra = {}
        for dtype in (torch.float32, torch.float64):
            torch.set_default_dtype(dtype)
            torch.manual_seed(seed)
            mols, graphs, (tree_t, graph_t), orders, homos, lumos = MolGraph.tensorize(
                [[s, 0.0, 0.0] for s in specs], vocab, common_atom_vocab)
            tree_np = [np.asarray(x.numpy()) for x in tree_t[:-1]] + [tree_t[-1]]
            graph_np = [np.asarray(x.numpy()) for x in graph_t[:-1]] + [graph_t[-1]]

            class A:
                pass
            a = A()
            a.vocab, a.atom_vocab, a.rnn_type, a.embed_size, a.hidden_size = vocab, common_atom_vocab, rnn, H, H
            a.depthT, a.depthG, a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = dT, dG, iT, iG, 0.0, L, tie
            if dec == "hier":
                model = PV.HierPropertyVAE(a)
                sd = seeded_state_dict(vae_param_shapes(rnn, H, L, n_motif, n_attach), seed)
                if tie:
                    sd = tied_state_dict(sd)
                res = model.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=False)
                assert not res.unexpected_keys, res.unexpected_keys
            else:
                model = PV.PropertyVAE(a)
                shapes = OrderedDict((k, tuple(p.shape)) for k, p in model.named_parameters())
                sd = seeded_state_dict(shapes, seed)
                with torch.no_grad():
                    for k, p in model.named_parameters():
                        p.copy_(torch.from_numpy(sd[k]).to(dtype))
                owner = {p.data_ptr(): k for k, p in reversed(list(model.named_parameters()))}
                extra["sd_keys"] = np.array(list(model.state_dict().keys()))
                extra["sd_src"] = np.array([owner.get(v.data_ptr(), "") for v in model.state_dict().values()])
                extra["param_names"] = np.array([k for k, _ in model.named_parameters()])
            model = model.to(dtype).eval()
            rec = {}

            def zip_spy(tup_list, is_concat=False):
                cols = list(zip(*tup_list))
                rec["mol"].append([int(x) if isinstance(x, int) else int(x.reshape(-1)[0]) for x in cols[1]])
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
            tensors = make_cuda((tree_np, graph_np))
            for vname, kind, beta, w in VARIANTS:
                model.zero_grad()
                root = model.encoder(tensors[0], tensors[1])[0] if dec == "hier" else model.encoder(tensors[0])[0]
                mean, pre_var = model.R_mean(root), model.R_var(root)
                lv = -torch.abs(pre_var)
                kl = -0.5 * (1.0 + lv - mean * mean - torch.exp(lv)).sum(dim=1)
                parts, logpq = [], []
                for k in range(K):
                    rec.clear()
                    rec["mol"] = []
                    e = torch.from_numpy(eps[k]).to(dtype)
                    z = mean + torch.exp(lv / 2) * e
                    d(mols, (z, z, z), graphs, tensors, orders)
                    rows_of = [("topo", 0), ("cls", 1), ("icls", 1)] + ([("assm", 2)] if "assm" in rec else [])
                    cols = []
                    for which, call in rows_of:
                        mol = torch.as_tensor(rec["mol"][call], dtype=torch.long)
                        cols.append(torch.zeros(B, dtype=dtype).index_add(0, mol, rec[which]))
                    if len(cols) < 4:
                        cols.append(torch.zeros(B, dtype=dtype))
                    parts.append(torch.stack(cols, dim=1))
                    logpq.append(-0.5 * (z * z).sum(dim=1) + 0.5 * (e * e + lv).sum(dim=1))
                parts, logpq = torch.stack(parts), torch.stack(logpq)
                loss = objective(kind, beta, w, parts, logpq, kl)
                loss.backward()
                runs[(vname, dtype)] = dict(
                    loss=float(loss.detach()), parts=parts.detach().numpy().astype(np.float64),
                    logpq=logpq.detach().numpy().astype(np.float64), kl=kl.detach().numpy().astype(np.float64),
                    grads={k: (p.grad.detach().numpy().astype(np.float32) if p.grad is not None else None)
                           for k, p in model.named_parameters()})
            for h in hooks:
                h.remove()
            D.zip_tensors = real_zip
        torch.set_default_dtype(torch.float32)

        ll = np.load(os.path.join(HERE, "mol_likelihood", name + ".npz"))
        for vname, kind, beta, w in VARIANTS:
            r32, r64 = runs[(vname, torch.float32)], runs[(vname, torch.float64)]
            # the parts of the likelihood fixture are those of this run (same batch, same draws)
            assert np.abs(r64["parts"] - ll["parts"]).max() <= 1e-5 * np.abs(ll["parts"]).max(), (name, vname)
            out = dict(extra)
            gmax = max(np.abs(g).max() for g in r64["grads"].values() if g is not None)
            dist = 0.0
            for k in r64["grads"]:
                g32, g64 = r32["grads"][k], r64["grads"][k]
                assert (g32 is None) == (g64 is None), k
                if g64 is None:
                    continue
                out["grad32/" + k], out["grad64/" + k] = g32, g64
                if np.abs(g64).max() >= 1e-6 * gmax:
                    dist = max(dist, float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max()))
            worst[kind] = max(worst[kind], dist)
            out.update(loss32=np.float32(r32["loss"]), loss64=np.float32(r64["loss"]), loss=np.float64(r64["loss"]),
                       parts=r64["parts"], logpq=r64["logpq"], kl=r64["kl"], eps=eps,
                       weights=np.asarray(w if w is not None else [1.0] * B, np.float32), weighted=np.int32(w is not None),
                       beta=np.float64(beta), objective=np.array(kind), case=np.array(name), meta=ll["meta"],
                       decoder=np.array(dec), rnn=np.array(rnn))
            path = os.path.join(OUT, "%s__%s.npz" % (name, vname))
            np.savez_compressed(path, **out)
            print("%-18s %-10s loss %.6f (fp32 %.6f)  max fp32/fp64 gradient distance %.2e  -> %.1f KB" % (
                name, vname, r64["loss"], r32["loss"], dist, os.path.getsize(path) / 1024))
    print("largest fp32 / fp64 gradient distance (max-norm per tensor): elbo %.2e, iwae %.2e" % (worst["elbo"], worst["iwae"]))


if __name__ == "__main__":
    main()
