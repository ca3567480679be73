"""Fused multi-head attention core (``OP_ATTENTION``): ``O = softmax(scale Q K^T + mask) V`` per head.

Inputs ``q [B, Tq, E]``, ``k [B, Tk, E]``, ``v [B, Tk, E]`` with ``E = heads * dh`` and head ``h`` at
columns ``[h*dh, (h+1)*dh)`` -- what a Linear writes, so the projections around the op stay ordinary
Linear ops (``FFModel.multihead_attention``) and no transpose is ever needed.  Output ``[B, Tq, E]``.
``causal`` (``Tq == Tk``): key ``j`` is visible to query ``i`` iff ``j <= i``.

On MI355X the flash-style kernels of ``csrc/kernels/attention.hip`` run it: no ``[Tq, Tk]`` matrix
reaches memory, and the only state kept for the backward is the per-row log-sum-exp (fp32
``[B, heads, Tq]``, allocated once in ``ctx.saved`` so a captured step replays on one address).
The backward is the true gradient of all three inputs (the framework's ``Softmax.backward`` is the
identity: it only ever sat in front of the cross-entropy loss).  The CPU path is the explicit
formula in fp32, its backward written out.
"""
from __future__ import annotations

import math

import torch

from flexmi.core.types import OperatorType
from flexmi.parallel.layout import Layout

from .base import Op, OpCtx, store
from . import _kernels as K


class Attention(Op):
    op_type = OperatorType.OP_ATTENTION
    name_prefix = "Attention"
    HIP_HEAD_DIMS = (32, 64, 128)

    def __init__(self, model, q, k, v, heads, causal=False, scale=None, name=None):
        super().__init__(model, [q, k, v], name)
        heads = int(heads)
        if not (len(q.dims) == len(k.dims) == len(v.dims) == 3):
            raise ValueError(f"Attention: q, k, v must be [B, T, E], got {q.dims}, {k.dims}, {v.dims}")
        B, Tq, E = q.dims
        if tuple(k.dims) != tuple(v.dims) or k.dims[0] != B or k.dims[2] != E:
            raise ValueError(f"Attention: q {tuple(q.dims)} needs k and v of one shape [B, Tk, E], got "
                             f"{tuple(k.dims)} and {tuple(v.dims)}")
        if heads < 1 or E % heads != 0:
            raise ValueError(f"Attention: embedding width {E} is not a multiple of heads = {heads}")
        if causal and k.dims[1] != Tq:
            raise ValueError(f"Attention: causal needs Tq == Tk, got {Tq} and {k.dims[1]}")
        self.heads, self.dh, self.causal = heads, E // heads, bool(causal)
        self.scale = float(scale) if scale is not None else 1.0 / math.sqrt(self.dh)
        if self.name is None:
            self.name = self.auto_name(str(heads))
        self._finish([tuple(q.dims)])

    def check_hip(self):
        """The limits of the HIP kernels (csrc/kernels/attention.hip), raised at compile()."""
        if self.dh not in self.HIP_HEAD_DIMS:
            raise ValueError(f"Attention '{self.name}' has head dimension {self.dh}: the HIP kernels take "
                             f"{self.HIP_HEAD_DIMS}; the CPU backend has no limit")
        if self.heads > 65535:
            raise ValueError(f"Attention '{self.name}' has {self.heads} heads: the HIP kernels take at most 65535")

    def splittable_dims(self):
        return {0}

    def input_layouts(self, pc):
        lo = Layout.from_pc(self.outputs[0].dims, pc)
        return [Layout(t.dims, lo.degrees, lo.holders) for t in self.inputs]

    def _heads(self, t):
        """[B, T, E] -> fp32 [B, heads, T, dh]"""
        return t.float().reshape(t.shape[0], t.shape[1], self.heads, self.dh).transpose(1, 2)

    def _probs(self, q, k):
        s = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        if self.causal:
            hidden = torch.ones(s.shape[-2:], dtype=torch.bool, device=s.device).triu(1)
            s = s.masked_fill(hidden, float("-inf"))
        s = s - s.amax(-1, keepdim=True)
        e = torch.exp(s)
        return e / e.sum(-1, keepdim=True)

    def forward(self, ctx: OpCtx):
        q, k, v = ctx.inputs
        y = ctx.outputs[0]
        if ctx.hip:
            lse = ctx.saved.get("lse")
            if lse is None or lse.numel() != q.shape[0] * self.heads * q.shape[1]:
                lse = ctx.saved["lse"] = torch.empty(q.shape[0], self.heads, q.shape[1], dtype=torch.float32,
                                                     device=q.device)
            K.attention_forward(q, k, v, y, lse, self.heads, self.causal, self.scale)
            return
        o = torch.matmul(self._probs(self._heads(q), self._heads(k)), self._heads(v))
        y.copy_(o.transpose(1, 2).reshape(y.shape))

    def backward(self, ctx: OpCtx):
        q, k, v = ctx.inputs
        dy = ctx.out_grads[0]
        g = list(ctx.in_grads) + [None] * (3 - len(ctx.in_grads))
        acc = list(ctx.in_grad_accumulate) + [False] * (3 - len(ctx.in_grad_accumulate))
        if all(x is None for x in g):
            return
        if ctx.hip:
            K.attention_backward(q, k, v, ctx.outputs[0], dy, ctx.saved["lse"], g[0], g[1], g[2], acc, self.heads,
                                 self.causal, self.scale)
            return
        qh, kh, vh, do = self._heads(q), self._heads(k), self._heads(v), self._heads(dy)
        p = self._probs(qh, kh)
        dp = torch.matmul(do, vh.transpose(-1, -2))
        ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * self.scale      # softmax backward, then the scale
        back = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)   # noqa: E731
        if g[0] is not None:
            store(g[0], back(torch.matmul(ds, kh)), acc[0])
        if g[1] is not None:
            store(g[1], back(torch.matmul(ds.transpose(-1, -2), qh)), acc[1])
        if g[2] is not None:
            store(g[2], back(torch.matmul(p.transpose(-1, -2), do)), acc[2])

    def flops(self, i, o):
        """Forward: the two products, 4 B heads Tq Tk dh, half of it under the causal mask."""
        B, Tq, E = i[0]
        return 4.0 * B * Tq * i[1][1] * E * (0.5 if self.causal else 1.0)
