"""Fused multi-head attention core (``OP_ATTENTION``): ``O = softmax(scale Q K^T + mask) V`` per head.

Inputs ``q [B, Tq, E]``, ``k [B, Tk, Ek]``, ``v [B, Tk, Ek]`` with ``E = heads * dh`` and head ``h`` at
columns ``[h*dh, (h+1)*dh)`` -- what a Linear writes, so the projections around the op stay ordinary
Linear ops (``FFModel.multihead_attention``) and no transpose is ever needed.  Output ``[B, Tq, E]``.
``causal`` (``Tq == Tk``): key ``j`` is visible to query ``i`` iff ``j <= i``.

``kv_heads`` (grouped-query / multi-query attention, default ``heads``, must divide it): ``Ek =
kv_heads * dh`` and query head ``h`` reads KV head ``h // G``, ``G = heads // kv_heads``; ``dk`` / ``dv``
are the sums over a group's query heads.  ``key_lengths``: a fourth input, int32 ``[B, 1]`` without a
gradient; key ``j`` of sample ``b`` is visible iff ``j < clamp(len[b], 0, Tk)`` (and ``j <= i`` when
causal).  Query rows are never masked (``torch.nn.MultiheadAttention``'s ``key_padding_mask``).  A row
without a visible key (``len[b] == 0``) has output 0 and adds nothing to any gradient; key rows at or past
the length get ``dk = dv = 0`` and their contents, NaN included, never reach a result.

On MI355X the flash-style kernels of ``csrc/kernels/attention.hip`` run it: no ``[Tq, Tk]`` matrix
reaches memory, and the only state kept for the backward is the per-row log-sum-exp (fp32
``[B, heads, Tq]``, allocated once in ``ctx.saved`` so a captured step replays on one address).  The
lengths are read on the device only, so a captured step replays with whatever its buffer then holds.
The backward is the true gradient of all three inputs (the framework's ``Softmax.backward`` is the
identity: it only ever sat in front of the cross-entropy loss).  The CPU path is the explicit
formula in fp32, its backward written out; padded key rows are selected away, never multiplied by 0.

``rope_base`` (rotary position embedding, default ``None``: no rotation, the op as it was): with a base
``theta`` (10000.0 is the usual one) row ``t`` of ``q`` and row ``t`` of ``k`` are rotated per head by the angles
``t * theta ** (-2 i / dh)``, ``i`` in ``[0, dh / 2)``, before the scores are formed; ``v`` and the output are
untouched.  The default pairs columns ``(i, i + dh / 2)`` (half-split: GPT-NeoX, Hugging Face Llama),
``rope_interleaved`` pairs ``(2 i, 2 i + 1)`` (GPT-J, RoFormer).  Positions are row indices, with ``causal``,
``kv_heads`` and ``key_lengths`` alike (right for right-padded batches); a KV head is rotated once however
many query heads read it.  ``dq`` / ``dk`` are the true gradients: those of the rotated rows, rotated back by
the transpose.  The cos / sin table (:func:`rope_table`) is computed once in float64 on the host, rounded to
fp32 and kept with the op; both backends read it, the HIP kernels from a device copy made at
``init_layers()``, rotating ``q`` / ``k`` on their way into the matrix instructions and ``dq`` / ``dk`` on their
way out of the accumulators: no extra pass over memory.  Not provided: partial rotary (``rotary_dim < dh``),
per-sample or offset positions, frequency scaling (NTK / YaRN), and the Keras / torch.fx / ONNX / C surfaces
and the native engine.
"""
from __future__ import annotations

import math

import torch

from flexmi.core.types import DataType, OperatorType
from flexmi.parallel.layout import Layout

from .base import Op, OpCtx, store
from . import _kernels as K


def rope_table(positions, dh, base):
    """fp32 ``[positions, dh]``: row ``t`` holds ``cos(t w_i)`` then ``sin(t w_i)``, ``w_i = base ** (-2 i / dh)``,
    ``i < dh / 2``, computed in float64 and rounded once.  A row is what one position needs, and its 16-byte
    pieces are the frequencies of the 16-byte chunks the kernels load of ``q`` and ``k``."""
    w = float(base) ** (-torch.arange(0, dh, 2, dtype=torch.float64) / dh)
    ang = torch.arange(positions, dtype=torch.float64)[:, None] * w[None, :]
    return torch.cat((ang.cos(), ang.sin()), 1).float()


def rope_rotate(x, table, interleaved, transpose=False):
    """``x [..., T, dh]`` with row ``t`` rotated by row ``t`` of ``table``; ``transpose``: by the inverse."""
    half = x.shape[-1] // 2
    c, s = table[:x.shape[-2], :half].to(x.dtype), table[:x.shape[-2], half:].to(x.dtype)
    if transpose:
        s = -s
    lo, hi = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :half], x[..., half:])
    lo, hi = lo * c - hi * s, hi * c + lo * s
    return torch.stack((lo, hi), -1).flatten(-2) if interleaved else torch.cat((lo, hi), -1)


class Attention(Op):
    op_type = OperatorType.OP_ATTENTION
    name_prefix = "Attention"
    HIP_HEAD_DIMS = (32, 64, 128)

    def __init__(self, model, q, k, v, heads, causal=False, scale=None, name=None, kv_heads=None, key_lengths=None,
                 rope_base=None, rope_interleaved=False):
        super().__init__(model, [q, k, v] + ([] if key_lengths is None else [key_lengths]), name)
        heads = int(heads)
        kv_heads = heads if kv_heads is None else int(kv_heads)
        if not (len(q.dims) == len(k.dims) == len(v.dims) == 3):
            raise ValueError(f"Attention: q, k, v must be [B, T, E], got {q.dims}, {k.dims}, {v.dims}")
        B, Tq, E = q.dims
        if heads < 1 or E % heads != 0:
            raise ValueError(f"Attention: embedding width {E} is not a multiple of heads = {heads}")
        if kv_heads < 1 or heads % kv_heads != 0:
            raise ValueError(f"Attention: kv_heads = {kv_heads} does not divide heads = {heads}")
        Ek = E // heads * kv_heads
        if tuple(k.dims) != tuple(v.dims) or k.dims[0] != B or k.dims[2] != Ek:
            raise ValueError(f"Attention: q {tuple(q.dims)} with kv_heads = {kv_heads} of {heads} heads needs k and v of one "
                             f"shape [B, Tk, {Ek}], got {tuple(k.dims)} and {tuple(v.dims)}")
        if causal and k.dims[1] != Tq:
            raise ValueError(f"Attention: causal needs Tq == Tk, got {Tq} and {k.dims[1]}")
        if key_lengths is not None and (tuple(key_lengths.dims) != (B, 1) or key_lengths.data_type != DataType.DT_INT32):
            raise ValueError(f"Attention: key_lengths must be an int32 tensor [{B}, 1], got {key_lengths.data_type.name} "
                             f"{tuple(key_lengths.dims)}")
        self.heads, self.kv_heads, self.dh, self.causal = heads, kv_heads, E // heads, bool(causal)
        if rope_base is not None and self.dh % 2 != 0:
            raise ValueError(f"Attention: rope_base needs an even head dimension, got {self.dh}")
        if rope_base is not None and not float(rope_base) > 0:
            raise ValueError(f"Attention: rope_base must be positive, got {rope_base}")
        self.rope_base = None if rope_base is None else float(rope_base)
        self.rope_interleaved = bool(rope_interleaved)
        # positions are row indices: the table depends on nothing a sample split changes
        self.rope = None if rope_base is None else rope_table(max(Tq, k.dims[1]), self.dh, self.rope_base)
        self.has_lengths = key_lengths is not None
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

    def prepare(self, ctx):
        """The rotary table at its fixed device address before any step can be captured."""
        if self.rope is not None and ctx.inputs and ctx.inputs[0] is not None:
            ctx.saved["rope"] = self.rope.to(ctx.inputs[0].device)

    def _rope(self, x, transpose=False):
        """fp32 heads [B, n, T, dh] rotated by their row index (``transpose``: gradients rotated back)."""
        return x if self.rope is None else rope_rotate(x, self.rope.to(x.device), self.rope_interleaved, transpose)

    def splittable_dims(self):
        return {0}

    def input_layouts(self, pc):
        lo = Layout.from_pc(self.outputs[0].dims, pc)
        # the lengths [B, 1] follow the sample split of the output (the only split there is)
        return [Layout(t.dims, lo.degrees[:len(t.dims)], lo.holders) for t in self.inputs]

    def _heads(self, t, n):
        """[B, T, n * dh] -> fp32 [B, n, T, dh]"""
        return t.float().reshape(t.shape[0], t.shape[1], n, self.dh).transpose(1, 2)

    def _kv(self, ctx):
        """K and V as fp32 [B, heads, Tk, dh] (a KV head repeated for its group, rows at or past the
        sample's length selected to 0) and the visibility [B or 1, 1, Tq or 1, Tk] of each key, or None."""
        k, v = ctx.inputs[1], ctx.inputs[2]
        Tq, Tk = ctx.inputs[0].shape[1], k.shape[1]
        vis = None
        if self.causal:
            vis = torch.ones(Tq, Tk, dtype=torch.bool, device=k.device).tril()[None, None]
        if self.has_lengths:
            live = torch.arange(Tk, device=k.device)[None, :] < ctx.inputs[3].reshape(-1, 1).clamp(0, Tk)    # [B, Tk]
            zero = torch.zeros((), dtype=k.dtype, device=k.device)
            k, v = torch.where(live[:, :, None], k, zero), torch.where(live[:, :, None], v, zero)
            vis = live[:, None, None, :] if vis is None else vis & live[:, None, None, :]
        G = self.heads // self.kv_heads
        kh, vh = self._rope(self._heads(k, self.kv_heads)), self._heads(v, self.kv_heads)   # a KV head rotated once
        if G > 1:
            kh, vh = kh.repeat_interleave(G, 1), vh.repeat_interleave(G, 1)
        return kh, vh, vis

    def _probs(self, q, k, vis):
        s = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        if vis is not None:
            s = s.masked_fill(~vis, float("-inf"))
        mx = s.amax(-1, keepdim=True)
        e = torch.exp(s - torch.where(mx == float("-inf"), torch.zeros_like(mx), mx))   # a row without a key: all 0
        den = e.sum(-1, keepdim=True)
        return e / torch.where(den == 0, torch.ones_like(den), den)

    def forward(self, ctx: OpCtx):
        q, k, v = ctx.inputs[:3]
        y = ctx.outputs[0]
        if ctx.hip:
            lse = ctx.saved.get("lse")
            if lse is None or lse.numel() != q.shape[0] * self.heads * q.shape[1]:
                lse = ctx.saved["lse"] = torch.empty(q.shape[0], self.heads, q.shape[1], dtype=torch.float32,
                                                     device=q.device)
            K.attention_forward(q, k, v, y, lse, self.heads, self.causal, self.scale, self.kv_heads,
                                ctx.inputs[3] if self.has_lengths else None, ctx.saved.get("rope"), self.rope_interleaved)
            return
        kh, vh, vis = self._kv(ctx)
        o = torch.matmul(self._probs(self._rope(self._heads(q, self.heads)), kh, vis), vh)
        y.copy_(o.transpose(1, 2).reshape(y.shape))

    def backward(self, ctx: OpCtx):
        q, k, v = ctx.inputs[:3]
        dy = ctx.out_grads[0]
        g = (list(ctx.in_grads) + [None] * 3)[:3]
        acc = (list(ctx.in_grad_accumulate) + [False] * 3)[:3]
        if all(x is None for x in g):
            return
        if ctx.hip:
            K.attention_backward(q, k, v, ctx.outputs[0], dy, ctx.saved["lse"], g[0], g[1], g[2], acc, self.heads,
                                 self.causal, self.scale, self.kv_heads, ctx.inputs[3] if self.has_lengths else None,
                                 ctx.saved.get("rope"), self.rope_interleaved)
            return
        qh, do = self._rope(self._heads(q, self.heads)), self._heads(dy, self.heads)
        kh, vh, vis = self._kv(ctx)
        p = self._probs(qh, kh, vis)
        dp = torch.matmul(do, vh.transpose(-1, -2))
        ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * self.scale      # softmax backward, then the scale
        back = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)   # noqa: E731
        # [B, heads, Tk, dh] -> the sum over each KV head's group
        group = lambda t: t.reshape(t.shape[0], self.kv_heads, -1, *t.shape[2:]).sum(2)   # noqa: E731
        if g[0] is not None:
            store(g[0], back(self._rope(torch.matmul(ds, kh), True)), acc[0])
        if g[1] is not None:
            store(g[1], back(self._rope(group(torch.matmul(ds.transpose(-1, -2), qh)), True)), acc[1])
        if g[2] is not None:
            store(g[2], back(group(torch.matmul(p.transpose(-1, -2), do))), acc[2])

    def flops(self, i, o):
        """Forward: the two products, 4 B heads Tq Tk dh (every query head does them whatever kv_heads
        is), half of it under the causal mask; the lengths are data and not counted."""
        B, Tq, E = i[0]
        return 4.0 * B * Tq * i[1][1] * E * (0.5 if self.causal else 1.0)
