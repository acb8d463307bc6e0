#!/usr/bin/env python3
"""Golden fixtures for the property heads and the latent search, produced by RUNNING THE REFERENCE:

    python tests/golden/make_golden_propopt.py          (build container only; needs the reference checkout)

propopt_*:   the reference's ``HierPropOptVAE(args)(*batch, beta, perturb_z=False)`` (ggpm/property_vae.py:130-254) on a
             synthetic batch, then ``total_loss.backward()``.  Recorded: total loss, every metric, every parameter gradient
             in full, the names of the parameters whose ``.grad`` is None, and the state_dict keys.
propsearch_*: the reference's ``soft_optimize`` / ``patience_optimize`` / ``hard_optimize`` (ggpm/property_control.py)
             called directly on seeded heads, latents and targets, in fp32 and in fp64.  Recorded: final latents,
             predictions on them, per-molecule loop bodies (forward hooks on the heads), and the smallest relative margin
             of every stopping decision and sign test of the fp64 run (tests/property_oracle.py restates the search and
             must reproduce the reference's fp64 run exactly in its decisions).  Seeds are kept only when that margin is
             >= 1e-3, so that an fp32 reordering cannot flip a decision.
Written to tests/golden/property/.  Fixtures are DATA; no reference source text is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.path for ggpm_amd / tests)
import make_golden_vae as mgv  # noqa: E402

import torch  # noqa: E402

from ggpm_amd import synth  # noqa: E402
from ggpm_amd.params import seeded_state_dict  # noqa: E402
from ggpm_amd.vocab import IndexPairVocab  # noqa: E402
import property_oracle as po  # noqa: E402
from property_fixtures import head_shapes, propopt_state_dict, targets  # noqa: E402

PROPOPT_CASES = [
    # name, rnn, H, latent, depthT, depthG, diterT, diterG, B, motifs, n_motif, tie, linear_hidden, loss_scaling, seed
    ("propopt_gru_s50", "GRU", 16, 8, 3, 3, 1, 2, 3, (2, 5), 11, False, 16, False, 50),
    ("propopt_lstm_s51", "LSTM", 24, 8, 2, 4, 1, 3, 3, (1, 5), 11, True, [12, 12], False, 51),
    ("propopt_gru_s52", "GRU", 20, 8, 2, 3, 1, 2, 4, (2, 4), 11, False, [8, 8], True, 52),
    ("propopt_lstm_s53", "LSTM", 16, 8, 2, 2, 1, 2, 3, (1, 4), 11, True, [16, 16, 16], False, 53),
]

SEARCH_CASES = [
    # name-prefix, mode, latent, linear_hidden, patience, threshold, delta, lr, steps, B, first seed
    ("propsearch_soft", "soft", 24, [64, 64], 5, 0.1, 0.1, 1.0, 20, 20, 60),
    ("propsearch_patience", "patience", 24, [64, 64], 5, 0.1, 0.1, 1.0, 20, 20, 70),
    ("propsearch_patience", "patience", 24, 128, 0.5, 0.1, 0.1, 1.0, 20, 20, 80),
    ("propsearch_fixed", "fixed", 24, [64, 64], 5, 0.1, 0.1, 1.0, 20, 20, 90),
    ("propsearch_soft", "soft", 24, 128, 5, 0.1, 0.1, 1.0, 20, 20, 100),
]
MARGIN = 1e-3
ORACLE_CAP = 2000


def make_propopt():
    mg.import_reference()
    import ggpm.property_vae as PV
    from ggpm.mol_graph import MolGraph
    from ggpm.vocab import common_atom_vocab
    MolGraph.__init__ = mgv.patched_init
    for (name, rnn, H, L, dT, dG, iT, iG, B, motifs, n_motif, tie, hidden, scaling, seed) in PROPOPT_CASES:
        torch.set_default_dtype(torch.float32)
        torch.manual_seed(seed)
        n_attach = 3 * n_motif
        specs = synth.random_batch(seed, B, motifs=motifs, n_motif_vocab=n_motif, n_attach_vocab=n_attach)
        vocab = IndexPairVocab(n_motif, n_attach)
        th, tl = targets(seed, B)
        mols, graphs, (tree_t, graph_t), orders, homos, lumos = MolGraph.tensorize(
            [[s, float(h), float(lu)] for s, h, lu in zip(specs, th, tl)], vocab, common_atom_vocab)
        tree_np = [np.asarray(x.numpy()) for x in tree_t[:-1]] + [tree_t[-1]]
        graph_np = [np.asarray(x.numpy()) for x in graph_t[:-1]] + [graph_t[-1]]

        class A:
            pass
        a = A()
        a.vocab, a.atom_vocab, a.rnn_type, a.embed_size, a.hidden_size = vocab, common_atom_vocab, rnn, H, H
        a.depthT, a.depthG, a.diterT, a.diterG, a.dropout, a.latent_size, a.tie_embedding = dT, dG, iT, iG, 0.0, L, tie
        a.linear_hidden_size, a.property_optim_step = hidden, 20
        if scaling:
            a.loss_scaling = True
        model = PV.HierPropOptVAE(a)
        sd = propopt_state_dict(rnn, H, L, n_motif, n_attach, tie, hidden, scaling, seed)
        res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(k.startswith(("decoder.rnn_cell.", "decoder.E_assm.")) for k in res.missing_keys), res.missing_keys
        seen = []
        hook = model.R_mean.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
        loss, metrics, clipped = model(mols, graphs, (tree_np, graph_np), orders, homos, lumos, beta=0.1, perturb_z=False)
        hook.remove()
        assert not clipped and len(seen) == 1
        loss.backward()
        out = {"loss": np.asarray(loss.detach().numpy(), np.float64).reshape(()),
               "metric_names": np.array(list(metrics.keys())),
               "metric_values": np.array([float(v) for v in metrics.values()], np.float64),
               "none_grads": np.array(sorted(k for k, p in model.named_parameters() if p.grad is None)),
               "state_keys": np.array(list(model.state_dict().keys())),
               "param_names": np.array([k for k, _ in model.named_parameters()]),
               "t_homo": th, "t_lumo": tl, "latent": seen[0].numpy()}
        for k, prm in model.named_parameters():
            if prm.grad is not None:
                out["grad/" + k] = prm.grad.numpy()
        out["meta"] = np.array([H, L, dT, dG, iT, iG, B, n_motif, n_attach, seed, motifs[0], motifs[1], int(tie),
                                int(scaling)], dtype=np.int64)
        out["linear_hidden"] = np.array([hidden] if isinstance(hidden, int) else hidden, np.int64)
        out["linear_hidden_is_int"] = np.array(isinstance(hidden, int))
        out["rnn"] = np.array(rnn)
        path = os.path.join(HERE, "property", name + ".npz")
        np.savez_compressed(path, **out)
        print("%-18s loss=%.6f metrics=%s none=%s -> %.1f KB" % (
            name, float(out["loss"]), np.round(out["metric_values"], 4).tolist(), out["none_grads"].tolist(),
            os.path.getsize(path) / 1024))


def search_inputs(seed, latent, hidden, B):
    half = latent // 2
    sd = seeded_state_dict(head_shapes(half, hidden), seed, bias_scale=0.3)
    rs = np.random.RandomState(seed + 1)
    z = rs.standard_normal((B, latent)).astype(np.float32)
    th, tl = targets(seed, B)
    return sd, z, th, tl


def run_reference(mode, sd, z, th, tl, half, hidden, args, dtype):
    from ggpm.property_optimizer import PropertyOptimizer
    from ggpm.property_control import PropertyVAEOptimizer

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.property_optim = PropertyOptimizer(half, hidden, 0.0)

    m = M()
    m.property_optim.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dtype).eval()
    calls = []
    m.property_optim.register_forward_hook(lambda mod, inp, out: calls.append(inp[2][0].data_ptr()))
    opt = PropertyVAEOptimizer(m, args)
    fn = {"soft": opt.soft_optimize, "patience": opt.patience_optimize, "fixed": opt.hard_optimize}[mode]
    zt = torch.from_numpy(z).to(dtype)
    tht, tlt = torch.from_numpy(th).to(dtype), torch.from_numpy(tl).to(dtype)
    with torch.enable_grad():
        zo = fn(homo_vecs=zt[:, :half], lumo_vecs=zt[:, half:], homo_targets=tht, lumo_targets=tlt)
    zo = zo.detach()
    with torch.no_grad():
        ph, pl = m.property_optim.predict(zo[:, :half], zo[:, half:])
    B = z.shape[0]
    if mode == "fixed":
        steps = np.full(B, len(calls), np.int64)
    else:
        ptrs = [tht[i].data_ptr() for i in range(B)]
        steps = np.array([sum(1 for c in calls if c == p) for p in ptrs], np.int64)
    return zo.numpy(), ph.numpy(), pl.numpy(), steps


def make_propsearch():
    mg.import_reference()
    done = {}
    for (prefix, mode, latent, hidden, patience, thr, delta, lr, steps, B, seed0) in SEARCH_CASES:
        half = latent // 2

        class Args:
            pass
        args = Args()
        args.property_optim_step, args.patience, args.optimize_type = steps, patience, mode
        args.property_delta, args.patience_threshold, args.latent_lr = delta, thr, lr
        for seed in range(seed0, seed0 + 200):
            sd, z, th, tl = search_inputs(seed, latent, hidden, B)
            homo, lumo = po.head_layers(sd, "homo_linear"), po.head_layers(sd, "lumo_linear")
            marg = po.Margins()
            z64, p64, n64, st64 = po.search(mode, homo, lumo, z.astype(np.float64), half, th, tl, lr, steps, delta,
                                            patience, thr, ORACLE_CAP, np.float64, marg)
            if (st64 != po.DONE).any() or marg.min < MARGIN or not np.isfinite(z64).all():
                continue
            if mode != "fixed" and patience >= 1 and n64.max() < 3:
                continue                 # want trajectories of several steps
            r32 = run_reference(mode, sd, z, th, tl, half, hidden, args, torch.float32)
            r64 = run_reference(mode, sd, z.astype(np.float64), th.astype(np.float64), tl.astype(np.float64), half, hidden,
                                args, torch.float64)
            assert (r64[3] == n64).all() and (r32[3] == n64).all(), (seed, r64[3], r32[3], n64)
            assert np.abs(r64[0] - z64).max() <= 1e-9 * max(1.0, np.abs(z64).max()), seed
            break
        else:
            raise RuntimeError("no seed with margins >= %g for %s" % (MARGIN, prefix))
        name = "%s_s%d" % (prefix, seed)
        out = {"mode": np.array(mode), "latent": np.int64(latent), "linear_hidden": np.array(
            [hidden] if isinstance(hidden, int) else hidden, np.int64),
            "params": np.array([patience, thr, delta, lr], np.float64), "steps": np.int64(steps), "seed": np.int64(seed),
            "z": z, "t_homo": th, "t_lumo": tl,
            "z_ref": r32[0], "pred_ref": np.stack([r32[1], r32[2]]), "z_ref64": r64[0], "pred_ref64": np.stack([r64[1], r64[2]]),
            "steps_ref": r32[3], "min_margin": np.float64(marg.min), "state_keys": np.array(list(sd.keys()))}
        for k, v in sd.items():
            out["w/" + k] = v
        path = os.path.join(HERE, "property", name + ".npz")
        np.savez_compressed(path, **out)
        done[name] = True
        print("%-24s steps=%s margin=%.2e -> %.1f KB" % (name, r32[3].tolist(), marg.min, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    which = sys.argv[1:] or ["propopt", "propsearch"]
    if "propsearch" in which:
        make_propsearch()
    if "propopt" in which:
        make_propopt()
