"""CPU restatement (numpy, any float dtype) of the property heads and the latent search of csrc/property.hip -- the
arithmetic of ggpm/property_optimizer.py and ggpm/property_control.py:65-180, written out so that the tests can pin it
against the reference's own outputs (tests/golden/propsearch_*.npz) and check the HIP kernels against it.

Heads are lists of (W [out, in], b [out]) in nn.Linear layout; the last one is Linear(w, 1)."""
import numpy as np

from golden_utils import dropout_keep

SITE_HOMO, SITE_LUMO = 16, 20          # include/ggpm_hip.h GGPM_SITE_PROP_HOMO / _LUMO
DONE, CAPPED = 0, 1
MODES = ("fixed", "soft", "patience")


def head_layers(sd, prefix, dtype=np.float64):
    """[(W, b), ...] of ``<prefix>.linear.{0,3,6,...}`` in a state dict of numpy arrays / tensors."""
    out, i = [], 0
    while "%s.linear.%d.weight" % (prefix, i) in sd:
        W, b = sd["%s.linear.%d.weight" % (prefix, i)], sd["%s.linear.%d.bias" % (prefix, i)]
        out.append((np.asarray(W, dtype=dtype), np.asarray(b, dtype=dtype)))
        i += 3
    return out


def head_forward(layers, x, masks=None, scale=1.0):
    """-> (out [B], inputs of every Linear).  masks[i]: keep mask of hidden layer i's output (None: no dropout)."""
    acts, h = [x], x
    for i, (W, b) in enumerate(layers[:-1]):
        a = np.maximum(h @ W.T + b, 0)
        if masks is not None:
            a = np.where(masks[i], a * a.dtype.type(scale), 0).astype(a.dtype)
        acts.append(a)
        h = a
    W, b = layers[-1]
    return (h @ W.T + b)[:, 0], acts


def head_backward(layers, acts, gout, scale=1.0):
    """d out = gout [B] -> (dx [B, in], [(dW, db), ...])."""
    D = gout[:, None]
    grads = [None] * len(layers)
    dx = None
    for i in range(len(layers) - 1, -1, -1):
        W, _ = layers[i]
        X = acts[i]
        grads[i] = (D.T @ X, D.sum(0))
        dx = D @ W
        if i > 0:
            D = np.where(X > 0, dx * dx.dtype.type(scale), 0).astype(dx.dtype)     # x = dropout(relu(pre)) > 0 <=> active
    return dx, grads


def heads_masks(B, layers, p, seed, site):
    if p <= 0:
        return None
    return [dropout_keep(B, W.shape[0], p, seed[0], seed[1], site + i) for i, (W, _) in enumerate(layers[:-1])]


def heads_step(homo, lumo, z, half, t_h, t_l, p=0.0, seed=(0, 0), dloss=(1.0, 1.0)):
    """The heads' forward + backward on z [B, >= 2 half] -> dict(pred, loss, dz, grads_homo, grads_lumo)."""
    B = z.shape[0]
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    out = {"pred": [], "loss": [], "dz": np.zeros_like(z), "grads": []}
    for hi, (layers, t, site) in enumerate(((homo, t_h, SITE_HOMO), (lumo, t_l, SITE_LUMO))):
        x = z[:, hi * half:(hi + 1) * half]
        o, acts = head_forward(layers, x, heads_masks(B, layers, p, seed, site), scale)
        out["pred"].append(o)
        out["loss"].append(((o - t) ** 2).mean())
        dx, g = head_backward(layers, acts, (2.0 / B) * (o - t) * dloss[hi], scale)
        out["dz"][:, hi * half:(hi + 1) * half] = dx
        out["grads"].append(g)
    return out


class Margins:
    """Smallest relative margin of every decision a search made (sign tests and stopping rules)."""

    def __init__(self):
        self.min = np.inf

    def add(self, m):
        self.min = min(self.min, float(np.min(m)) if np.size(m) else np.inf)


def _rel(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.nan_to_num(d, nan=np.inf)


def search(mode, homo, lumo, z, half, t_h, t_l, lr, steps, delta, patience, threshold, max_steps, dtype=np.float64,
           margins=None):
    """The latent search, per the contract of ggpm_property_latent_search -> (z_out, (pred_h, pred_l), steps [B],
    status [B])."""
    dt = np.dtype(dtype).type
    homo = [(W.astype(dt), b.astype(dt)) for W, b in homo]
    lumo = [(W.astype(dt), b.astype(dt)) for W, b in lumo]
    z = np.array(z, dtype=dt)
    t = (np.asarray(t_h, dtype=dt), np.asarray(t_l, dtype=dt))
    lr, delta, threshold, patience = dt(lr), dt(delta), dt(threshold), dt(patience)
    B = z.shape[0]
    heads = (homo, lumo)
    cols = (slice(0, half), slice(half, 2 * half))
    n_steps = np.zeros(B, np.int64)
    status = np.zeros(B, np.int64)

    def grad_update(v, tt, norm):
        """One signed update of every row of v (targets tt = (t_h, t_l) of those rows), both heads."""
        new = v.copy()
        for hi in range(2):
            x = v[:, cols[hi]]
            o, acts = head_forward(heads[hi], x)
            if margins is not None:
                margins.add(_rel(o, tt[hi]))
            dx, _ = head_backward(heads[hi], acts, dt(norm) * (o - tt[hi]))
            s = np.where(o < tt[hi], dt(-1), dt(1))
            new[:, cols[hi]] = x - (s * lr)[:, None] * dx
        return new

    if mode == "fixed":
        for _ in range(min(steps, max_steps)):
            z = grad_update(z, t, dt(2.0 / B))
        n_steps[:] = min(steps, max_steps)
        status[:] = CAPPED if steps > max_steps else DONE
    else:
        for r in range(B):
            v = z[r:r + 1].copy()
            pat, prev, n, stopped = patience, dt(0), 0, False
            while pat > 0 and n < max_steps:
                o = [head_forward(heads[hi], v[:, cols[hi]])[0][0] for hi in range(2)]
                loss = (o[0] - t[0][r]) ** 2 + (o[1] - t[1][r]) ** 2
                n += 1
                if mode == "soft":
                    if margins is not None:
                        margins.add(_rel(loss, delta))
                    if loss <= delta:
                        stopped = True
                        break
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.abs(loss - prev) / prev
                gt, le = bool(loss > prev), bool(ratio <= threshold)
                if margins is not None and prev > 0:
                    m_gt, m_le = _rel(loss, prev), _rel(ratio, threshold)
                    margins.add(max(m_gt if gt else 0, m_le if le else 0) if (gt or le) else min(m_gt, m_le))
                pat = pat - dt(1) if (gt or le) else patience
                prev = loss
                v = grad_update(v, (t[0][r:r + 1], t[1][r:r + 1]), dt(2.0))
            z[r] = v[0]
            n_steps[r] = n
            status[r] = CAPPED if (not stopped and pat > 0 and n >= max_steps) else DONE
    preds = tuple(head_forward(heads[hi], z[:, cols[hi]])[0] for hi in range(2))
    return z, preds, n_steps, status
