"""HOMO / LUMO property heads -- reference ggpm/property_optimizer.py (PropertyOptimizer, PropertyRegressor) and
ggpm/loss_weigh.py (LossWeigh).

Same constructor arguments, sub-module names and ``state_dict`` keys as the reference (``homo_linear.linear.0.weight``,
``...linear.3...``, ``...linear.6...``).  The two heads run as ONE autograd node over the latent: one launch forward
(both heads, their predictions and batch-mean MSEs), one launch backward (d latent and every weight / bias gradient),
csrc/property.hip.  There is no CPU path: the tensors must be fp32 on the GPU, and shapes outside the kernels'
envelope raise NotImplementedError.
"""
from __future__ import annotations

import ctypes
from typing import List, Union

import torch
import torch.nn as nn

from . import functional as F_

MAX_LINEAR, MAX_IN, MAX_WIDTH, MAX_B = 5, 256, 512, 1024


class PropHeadC(ctypes.Structure):
    _fields_ = [("n_linear", ctypes.c_int), ("width", ctypes.c_int * (MAX_LINEAR + 1)),
                ("W", ctypes.c_void_p * MAX_LINEAR), ("b", ctypes.c_void_p * MAX_LINEAR)]


class PropHeadGradsC(ctypes.Structure):
    _fields_ = [("dW", ctypes.c_void_p * MAX_LINEAR), ("db", ctypes.c_void_p * MAX_LINEAR), ("accumulate", ctypes.c_int)]


class PropertyRegressor(nn.Module):
    """``Linear -> ReLU -> Dropout`` over the hidden widths, then ``Linear(w, 1)`` (reference layout)."""

    def __init__(self, hidden_size: list, dropout: float):
        super().__init__()
        self.linear = nn.ModuleList()
        for idx in range(len(hidden_size) - 1):
            self.linear.extend([nn.Linear(hidden_size[idx], hidden_size[idx + 1]), nn.ReLU(), nn.Dropout(dropout)])
        self.linear.append(nn.Linear(hidden_size[-1], 1))

    def linears(self) -> List[nn.Linear]:
        return [m for m in self.linear if isinstance(m, nn.Linear)]

    @property
    def dropout(self) -> float:
        drops = [m.p for m in self.linear if isinstance(m, nn.Dropout)]
        return float(drops[0]) if drops else 0.0

    def forward(self, x):
        raise NotImplementedError("PropertyRegressor runs inside PropertyOptimizer (both heads in one launch); "
                                  "call PropertyOptimizer.forward / predict")

    def c_struct(self) -> PropHeadC:
        lins = self.linears()
        s = PropHeadC()
        s.n_linear = len(lins)
        s.width[0] = lins[0].in_features
        for i, lin in enumerate(lins):
            s.width[i + 1] = lin.out_features
            s.W[i] = lin.weight.data_ptr()
            s.b[i] = lin.bias.data_ptr()
        return s


def check_envelope(opt: "PropertyOptimizer", B: int) -> None:
    """NotImplementedError outside what csrc/property.hip was built for (there is no other path)."""
    for head in (opt.homo_linear, opt.lumo_linear):
        lins = head.linears()
        if not 2 <= len(lins) <= MAX_LINEAR:
            raise NotImplementedError("property heads: %d Linear layers; the HIP kernels take 2 to %d (1 to %d hidden)"
                                      % (len(lins), MAX_LINEAR, MAX_LINEAR - 1))
        if lins[0].in_features > MAX_IN:
            raise NotImplementedError("property heads: input width %d > %d" % (lins[0].in_features, MAX_IN))
        if any(lin.out_features > MAX_WIDTH for lin in lins[:-1]):
            raise NotImplementedError("property heads: hidden widths above %d are not supported" % MAX_WIDTH)
        for lin in lins:
            for t in (lin.weight, lin.bias):
                if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                    raise NotImplementedError("property heads: weights must be contiguous fp32 on the GPU")
    if B > MAX_B:
        raise NotImplementedError("property heads: batch %d > %d" % (B, MAX_B))


def _dropout_seed():
    from .fused import _dropout_seed as seed
    return seed()


class _PropertyHeads(torch.autograd.Function):
    """(z [B, ld], t_homo [B], t_lumo [B], *weights) -> (pred_homo [B], pred_lumo [B], mse_homo, mse_lumo): both heads in
    one launch each way.  The predictions are returned for reading (non-differentiable); the losses carry the gradient.
    Parameter gradients are written by the backward launch itself: straight into ``.grad`` (added into an existing one)
    when ``functional.can_publish`` allows -- in stream order on the current stream, so nothing else is needed to order
    them --, else returned through autograd.  (Unlike _KLHead there is no second stream: d latent and the
    parameter gradients come out of the same launch.)"""

    @staticmethod
    def forward(ctx, z, t_homo, t_lumo, opt, p, seed, *params):
        from . import _lib
        B, ld = z.shape
        half = opt.input_size
        heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
        lib = _lib.load()
        ws_bytes = lib.ggpm_property_heads_workspace_bytes(B, half, ctypes.byref(heads[0]), ctypes.byref(heads[1]))
        if ws_bytes == 0:
            raise RuntimeError("ggpm_amd: property heads: bad shapes")
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=z.device)
        pred = torch.empty(2, B, dtype=torch.float32, device=z.device)
        loss = torch.empty(2, dtype=torch.float32, device=z.device)
        _lib.check(lib.ggpm_property_heads_forward(B, F_._p(z), ld, half, ctypes.byref(heads[0]), ctypes.byref(heads[1]),
                                                   F_._p(t_homo), F_._p(t_lumo), float(p), seed[0], seed[1], F_._p(pred),
                                                   F_._p(loss), F_._p(ws), ws_bytes, F_._stream()),
                   "property_heads_forward")
        ctx.save_for_backward(z, t_homo, t_lumo, pred, ws)
        ctx.opt, ctx.p, ctx.params = opt, float(p), params
        ph, pl = pred[0], pred[1]
        ctx.mark_non_differentiable(ph, pl)
        return ph, pl, loss[0], loss[1]

    @staticmethod
    def backward(ctx, d_ph, d_pl, d_lh, d_ll):
        from . import _lib
        z, t_homo, t_lumo, pred, ws = ctx.saved_tensors
        B, ld = z.shape
        opt, params = ctx.opt, ctx.params
        dev = z.device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        dloss = torch.stack([d_lh if d_lh is not None else zero, d_ll if d_ll is not None else zero]).float().contiguous()
        dz = torch.zeros_like(z) if ctx.needs_input_grad[0] else None
        publish = F_.can_publish(*params) and all(ctx.needs_input_grad[6:])
        grads, structs, out = [], [], []
        for hi, head in enumerate((opt.homo_linear, opt.lumo_linear)):
            lins = head.linears()
            hp = [t for lin in lins for t in (lin.weight, lin.bias)]
            gs = PropHeadGradsC()
            have = [q.grad is not None for q in hp]
            acc = publish and all(have) and all(q.grad.is_contiguous() and q.grad.dtype == torch.float32 for q in hp)
            gl = [q.grad if acc else torch.empty_like(q) for q in hp]
            for i in range(len(lins)):
                gs.dW[i], gs.db[i] = gl[2 * i].data_ptr(), gl[2 * i + 1].data_ptr()
            gs.accumulate = 1 if acc else 0
            structs.append(gs)
            grads.append((hp, gl, acc))
        heads = (opt.homo_linear.c_struct(), opt.lumo_linear.c_struct())
        _lib.check(_lib.load().ggpm_property_heads_backward(
            B, F_._p(z), ld, opt.input_size, ctypes.byref(heads[0]), ctypes.byref(heads[1]), F_._p(t_homo), F_._p(t_lumo),
            ctx.p, F_._p(pred), F_._p(dloss), F_._p(ws), ws.numel() * 4, F_._p(dz), ld, 0, ctypes.byref(structs[0]),
            ctypes.byref(structs[1]), F_._stream()), "property_heads_backward")
        for hp, gl, acc in grads:
            if publish:
                if not acc:
                    main = torch.cuda.current_stream()
                    for q, g in zip(hp, gl):
                        F_._accumulate_grad(q, g, main)
                out.extend([None] * len(hp))
            else:
                out.extend(gl)
        return (dz, None, None, None, None, None) + tuple(out)


def _flatten(x: torch.Tensor, one_row: bool) -> torch.Tensor:
    return x[-1] if one_row else x


class PropertyOptimizer(nn.Module):
    """Two PropertyRegressor heads over the two latent halves (reference ggpm/property_optimizer.py)."""

    def __init__(self, input_size, hidden_size: Union[int, list], dropout):
        super().__init__()
        self.input_size = input_size
        hidden_size = [hidden_size] if isinstance(hidden_size, int) else list(hidden_size)
        hidden_size = [input_size] + hidden_size
        self.homo_linear = PropertyRegressor(hidden_size, dropout)
        self.lumo_linear = PropertyRegressor(hidden_size, dropout)
        self._dropout_seed = None           # (tests pin the dropout mask stream)

    def params(self):
        return [t for head in (self.homo_linear, self.lumo_linear) for lin in head.linears()
                for t in (lin.weight, lin.bias)]

    def compute_loss(self, outputs, targets):
        return torch.nn.MSELoss(reduction='mean')(outputs, targets)

    def forward_latent(self, z: torch.Tensor, targets):
        """The heads on the two halves of ``z [B, >= 2 input_size]`` (the layout HierPropOptVAE has) without a copy:
        -> (homo_loss, lumo_loss, homo_out [B], lumo_out [B])."""
        F_._need_gpu(z)
        if z.dim() != 2 or z.dtype != torch.float32:
            raise NotImplementedError("property heads: z must be a [B, L] fp32 matrix")
        z = z.contiguous()
        B = z.shape[0]
        check_envelope(self, B)
        t_h, t_l = (torch.as_tensor(t, dtype=torch.float32, device=z.device).reshape(-1).contiguous() for t in targets)
        if t_h.numel() != B or t_l.numel() != B:
            raise ValueError("property heads: %d rows, targets of %d / %d" % (B, t_h.numel(), t_l.numel()))
        p = self.homo_linear.dropout if self.training else 0.0
        seed = (self._dropout_seed or _dropout_seed()) if p > 0 else (0, 0)
        ph, pl, lh, ll = _PropertyHeads.apply(z, t_h, t_l, self, p, seed, *self.params())
        return lh, ll, ph, pl

    def forward(self, homo_vecs, lumo_vecs, targets):
        one_row = homo_vecs.dim() == 1
        z = torch.cat([homo_vecs.reshape(-1, self.input_size), lumo_vecs.reshape(-1, self.input_size)], dim=-1)
        lh, ll, ph, pl = self.forward_latent(z, targets)
        return lh, ll, _flatten(ph, one_row), _flatten(pl, one_row)

    def predict(self, homo_vecs, lumo_vecs):
        one_row = homo_vecs.dim() == 1
        z = torch.cat([homo_vecs.reshape(-1, self.input_size), lumo_vecs.reshape(-1, self.input_size)], dim=-1)
        zeros = torch.zeros(z.shape[0], dtype=torch.float32, device=z.device)
        _, _, ph, pl = self.forward_latent(z, (zeros, zeros))
        return _flatten(ph, one_row), _flatten(pl, one_row)


class LossWeigh(nn.Module):
    """Learned log-variance weights of the three losses (reference ggpm/loss_weigh.py): fp64 parameters, three scalar
    torch ops each -- kept in torch, not a hot path."""

    def __init__(self):
        super().__init__()
        self.homo_log_var = nn.Parameter(torch.zeros((1,), dtype=torch.float64), requires_grad=True)
        self.lumo_log_var = nn.Parameter(torch.zeros((1,), dtype=torch.float64), requires_grad=True)
        self.recon_log_var = nn.Parameter(torch.zeros((1,), dtype=torch.float64), requires_grad=True)

    def compute_recon_loss(self, loss):
        return loss * torch.exp(-self.recon_log_var) + self.recon_log_var

    def compute_prop_loss(self, homo_loss, lumo_loss):
        homo_loss = homo_loss * torch.exp(-self.homo_log_var) + self.homo_log_var
        lumo_loss = lumo_loss * torch.exp(-self.lumo_log_var) + self.lumo_log_var
        return homo_loss, lumo_loss
