"""CPU restatement of the tree-only models' training step: MotifEncoder, rsample, MotifDecoder.sum_forward (reference
ggpm/encoder.py:252-394, ggpm/decoder.py:475-899, ggpm/property_vae.py:64-127, 257-397), torch autograd in any dtype,
with the ``drop(site, x, step)`` hook of oracle/ref_decoder.py at every nn.Dropout the reference applies in training mode:

  "encoder.E_c", "encoder.E_i"                 MotifEncoder's embeddings (step None)
  "decoder.E_c", "decoder.W_o"                 IncEncoder's embedding and read-out, per decode step t
  "decoder.E_assm"                             enum_attach's E_assm rows, per decode step t
  "topoNN.2", "clsNN.2", "iclsNN.2"            the score heads (step None)

(MotifEncoder's tree_encoder.W_o Dropout acts on a node output nothing reads.)  The decode loop's bookkeeping is taken from
``DecodeSchedule.steps``, which tests/test_motif_vae_host.py pins to the reference's own recorded lists.
"""
import torch

from oracle import ref_encoder as R

F = torch.nn.functional
MAX_POS = 20


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def _nodrop(site, x, step):
    return x


def motif_encoder(p, rnn_type, depthT, tree, drop):
    """MotifEncoder.forward -> root vectors [B, H]."""
    fnode, fmess, agraph, bgraph = tree[:4]
    hnode = drop("encoder.E_c", p["E_c.0.weight"].index_select(0, fnode[:, 0]), None)
    hatt = drop("encoder.E_i", p["E_i.0.weight"].index_select(0, fnode[:, 1]), None)
    eye = torch.eye(MAX_POS, dtype=hnode.dtype)
    hmess = torch.cat([hatt.index_select(0, fmess[:, 0]), eye.index_select(0, fmess[:, 2])], dim=-1)
    _, mess = R.mpn_forward(p, "tree_encoder.", rnn_type, depthT, hnode, hmess, agraph, bgraph)
    return R.embed_root(p, mess, (hnode, hmess, agraph, bgraph), [st for st, _ in tree[-1]])


def motif_decoder(pd, rnn_type, diterT, tree, z, schedule, mask, drop):
    """MotifDecoder.sum_forward -> (loss, cls_acc, icls_acc, topo_acc, assm_acc)."""
    ph = _sub(pd, "hmpn.")
    B, H = schedule.batch_size, pd["topoNN.0.weight"].shape[0]
    L, dtype = z.shape[1], z.dtype
    init_vecs = z if L == H else R._affine(pd, "W_root", z)
    n_mess, N = tree[1].shape[0], tree[0].shape[0]
    dec = R.init_decoder_tensors(tree, B)
    zl = lambda n: torch.zeros(n, dtype=torch.long)      # noqa: E731
    htree = R.IncState(mess=R.rnn_init_state(rnn_type, n_mess, H, init_vecs, init_vecs),
                       emask=torch.cat([zl(n_mess), torch.ones(B, dtype=torch.long)]))
    prev = R.IncState(vmask=zl(1 + int(tree[4].max())))
    lt = lambda v: torch.tensor(list(v), dtype=torch.long)      # noqa: E731
    eye = torch.eye(MAX_POS, dtype=dtype)
    C = schedule.max_cls_size
    topo_vecs, cls_vecs, assm_vecs, assm_idx = [], [init_vecs], [], []
    for t, st in enumerate(schedule.steps):
        subnode, submess = lt(st["subnode"]), lt(st["submess"])
        htree.emask[submess] = 1
        cur = R.apply_tree_mask(dec, htree, prev)
        fnode, fmess, agraph, bgraph, _ = R._sub_tensor(cur, (subnode, submess))
        hnode = drop("decoder.E_c", ph["E_c.0.weight"].index_select(0, fnode[:, 0]), t)
        hmess = fmess if len(submess) == 0 else R._sub_messages(hnode, subnode, fmess, N)
        htree.node, htree.mess = R.inc_mpn_forward(ph, "tree_encoder.", rnn_type, diterT, (hnode, hmess, agraph, bgraph),
                                                   htree.mess, N, (subnode, submess),
                                                   drop=lambda site, x, step: drop("decoder.W_o", x, step), step=t)
        topo_vecs.append(htree.node.index_select(0, subnode))
        if st["cls_mess"]:
            cls_vecs.append(R._hidden(rnn_type, htree.mess).index_select(0, lt(st["cls_mess"])))
        for cands, icls, nth, i in st["assm"]:                  # enum_attach: no atom vectors
            n = len(cands)
            rows = drop("decoder.E_assm", ph["E_i.0.weight"].index_select(0, lt(list(icls) * n)), t)
            x = torch.cat([rows, eye[nth].expand(rows.shape[0], MAX_POS)], dim=-1)
            v = torch.relu(R._affine(pd, "matchNN.0", x))
            if len(icls) == 2:
                v = v.view(-1, 2, H).sum(dim=1)
            assm_vecs.append(F.pad(v, (0, 0, 0, C - v.shape[0])))
            assm_idx.append([i] * C)
    hd = lambda site, x, step: drop(site, x, step)      # noqa: E731
    tb, tl = schedule.topo()
    cb, cc, ci = schedule.cls()
    topo_vecs, cls_vecs = torch.cat(topo_vecs), torch.cat(cls_vecs)
    topo = R._head(pd, "topoNN", torch.cat([topo_vecs, z.index_select(0, lt(tb))], dim=-1), hd).squeeze(-1)
    x = torch.cat([cls_vecs, z.index_select(0, lt(cb))], dim=-1)
    cls = R._head(pd, "clsNN", x, hd)
    icls = R._head(pd, "iclsNN", x, hd) + mask.to(dtype).index_select(0, lt(cc))
    loss = F.binary_cross_entropy_with_logits(topo, lt(tl).to(dtype), reduction="sum")
    loss = loss + F.cross_entropy(cls, lt(cc), reduction="sum") + F.cross_entropy(icls, lt(ci), reduction="sum")
    topo_acc = ((topo >= 0).long() == lt(tl)).float().mean()
    cls_acc = (cls.argmax(-1) == lt(cc)).float().mean()
    icls_acc = (icls.argmax(-1) == lt(ci)).float().mean()
    if assm_vecs:
        av, ai = torch.stack(assm_vecs), torch.tensor(assm_idx, dtype=torch.long)
        assm = (R._affine(pd, "W_assm", av) * z.index_select(0, ai.reshape(-1)).view(ai.shape + (-1,))).sum(dim=-1)
        loss = loss + F.cross_entropy(assm, torch.zeros(len(assm_vecs), dtype=torch.long), reduction="sum")
        mx = assm.max(dim=-1)[0]
        assm_acc = (assm[:, 0] >= mx - 1e-9 * mx.abs()).float().mean()     # (equal real rows: ties are ties)
    else:
        assm_acc = torch.tensor(1.0)
    return loss / B, cls_acc, icls_acc, topo_acc, assm_acc


def _prop_head(p, prefix, x):
    i = 0
    while prefix + "linear.%d.weight" % (3 * (i + 1)) in p:
        x = torch.relu(R._affine(p, prefix + "linear.%d" % (3 * i), x))
        i += 1
    return R._affine(p, prefix + "linear.%d" % (3 * i), x).squeeze(-1)


def step(p, kind, rnn_type, depthT, diterT, tree, schedule, mask, beta, t_homo=None, t_lumo=None, drop=None):
    """One training step of PropertyVAE ('prop') or PropOptVAE ('prop-opt'), perturb_z=False: -> (total loss, metrics
    dict under the reference's keys).  ``p``: every parameter under its state_dict name (aliases may be missing)."""
    drop = drop or _nodrop
    root = motif_encoder(_sub(p, "encoder."), rnn_type, depthT, tree, drop)
    z, kl = R.rsample_kl(p, root)
    loss, wacc, iacc, tacc, sacc = motif_decoder(_sub(p, "decoder."), rnn_type, diterT, tree, z, schedule, mask, drop)
    loss = loss + beta * kl
    if kind == "prop":
        return loss, {'Loss': loss, 'KL:': kl, 'Word': wacc, 'I-Word': iacc, 'Topo': tacc, 'Assm': sacc}
    half = z.shape[1] // 2
    dt = z.dtype
    homo = F.mse_loss(_prop_head(p, "property_optim.homo_linear.", z[:, :half]), torch.as_tensor(t_homo).to(dt))
    lumo = F.mse_loss(_prop_head(p, "property_optim.lumo_linear.", z[:, half:]), torch.as_tensor(t_lumo).to(dt))
    if "loss_weigh.recon_log_var" in p:
        lw = lambda l, k: l * torch.exp(-p["loss_weigh." + k]) + p["loss_weigh." + k]      # noqa: E731
        loss, homo, lumo = lw(loss, "recon_log_var"), lw(homo, "homo_log_var"), lw(lumo, "lumo_log_var")
    total = loss + homo + lumo
    return total, {'Loss': total, 'KL': kl, 'Recs_Loss': loss, 'HOMO_MSE': homo, 'LUMO_MSE': lumo, 'Word': wacc,
                   'I-Word': iacc, 'Topo': tacc, 'Assm': sacc}


def run(golden, dtype=torch.float64, drop=None, model=None):
    """The oracle on a tests/motif_fixtures.MotifGolden case: -> (loss, metrics, {state_dict name: grad or None})."""
    from ggpm_amd.vocab import IndexPairVocab
    g = golden
    model = model if model is not None else g.model()
    sd = model.state_dict(keep_vars=True)
    leaves, p = {}, {}
    for k, v in sd.items():
        key = id(v)
        if key not in leaves:
            leaves[key] = v.detach().cpu().to(dtype if v.dtype == torch.float32 else v.dtype).clone().requires_grad_(True)
        p[k] = leaves[key]
    tensors, sch, _, homos, lumos = g.batch()
    tree = R.to_long_tensors(tensors[0])
    vocab = IndexPairVocab(g.n_motif, g.n_attach)
    mask = torch.as_tensor(vocab.mask).to(dtype) if not isinstance(vocab.mask, torch.Tensor) else vocab.mask.to(dtype)
    loss, metrics = step(p, g.kind, g.rnn, g.depthT, g.diterT, tree, sch, mask, g.beta, homos, lumos, drop)
    loss.backward()
    grads = {k: (p[k].grad if p[k].grad is not None else None) for k in sd}
    return loss.detach(), {k: float(v) for k, v in metrics.items()}, grads
