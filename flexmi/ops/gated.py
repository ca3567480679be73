"""Gated feed-forward layer, SwiGLU / GeGLU (``OP_GATED_LINEAR``).

On ``x [..., H]`` the op returns ``h [..., F]``::

    gu = x W^T            W is ONE parameter "kernel" [2F, H]: rows [0, F) = gate, rows [F, 2F) = up
    h  = act(g) * u       g = gu[:, :F], u = gu[:, F:]

``act`` is ``"silu"`` (SwiGLU, ``g * sigmoid(g)``) or ``"gelu"`` (GeGLU, the exact erf form ``g * Phi(g)``,
torch's default).  There is no bias.  Rows ``[0, F)`` of the kernel are Hugging Face Llama's
``gate_proj.weight``, rows ``[F, 2F)`` its ``up_proj.weight``.  Each half is initialised with the
distribution :meth:`FFModel.dense` gives a ``[F, H]`` kernel (Glorot with ``fan_out = F``); a
``kernel_initializer`` is used for both halves likewise.  The weight is an fp32 master with the usual
bf16 mirror (``ctx.wcompute``).  Every dim but the last may be split; the replicated weight's gradient
takes the ordinary bucketed all-reduce.  The op has its own type, so the executor's Linear-only paths
(fuse-below, fused SGD, grouped and deferred dW, the pipelined tail) do not apply.

Backward is the true gradient: ``dg = dh * u * act'(g)``, ``du = dh * act(g)``, ``dX (+)= [dg | du] W``,
``dW += [dg | du]^T x`` with ``silu'(g) = s (1 + g (1 - s))``, ``s = sigmoid(g)``, and ``gelu'(g) = Phi(g) +
g phi(g)``.

Rounding rule (both backends, both GPU forms): ``g`` and ``u`` are rounded to the compute dtype ONCE and
kept as ``gu [M, 2F]`` in ``ctx.saved`` (an op-private buffer allocated in the first forward); ``h`` is
computed in fp32 from the stored values and rounded once, and the backward reads the same stored values,
so the gradient is that of the function the forward evaluated.  In fp32 nothing is rounded.

On MI355X (``csrc/kernels/glu.hip``) the forward has two forms.  "fused": one MFMA kernel computes the
gate and the up tile from one staged ``x`` tile and multiplies them in registers (bf16; ``F % 4 == 0``, ``H
% 8 == 0``, 16-byte aligned rows).  "composed": the ordinary GEMM with ``N = 2F`` on the whole weight, then
the element-wise ``fm_glu_act_fwd`` (fp32, and every shape the fused kernel refuses).  :data:`FORM`
forces one; "auto" picks per call (see ``profiles/glu.txt`` for the measurement behind the choice).  The
backward is ``fm_glu_act_bwd`` writing ``dg`` and ``du`` side by side into an op-private ``dgu [M, 2F]``,
then ONE ordinary dX GEMM (``K = 2F``) and ONE ordinary weight-gradient GEMM.  The CPU path is one fp32
``matmul`` and the formulas above written out.
"""
from __future__ import annotations

import math

import torch

from flexmi.core.initializers import GlorotUniformInitializer, Initializer
from flexmi.core.types import OperatorType

from . import _kernels as K
from .base import Op, OpCtx, store

ACTIVATIONS = {"silu": 0, "gelu": 1}       # the kernels' activation codes
# forward form on the HIP backend: "auto" | "fused" | "composed" (tests run both on one shape)
FORM = "auto"
# what "auto" picks for bf16 operands the fused kernel takes (measured: profiles/glu.txt)
AUTO_BF16 = "fused"


class HalfRowsInitializer(Initializer):
    """``base`` with the parameters it gives a ``[rows / 2, cols]`` tensor, over the whole ``[rows, cols]``
    one: each half of the gated kernel gets the distribution of a ``dense(x, F)`` kernel (one counter
    stream, so the halves differ)."""

    def __init__(self, base):
        super().__init__()
        self.base = base

    def params(self, dims):
        return self.base.params((dims[0] // 2,) + tuple(dims[1:]))


def glu_act_torch(g, act):
    """fp32 ``act(g)`` and ``act'(g)`` written out (no autograd)"""
    if act == "silu":
        s = torch.sigmoid(g)
        return g * s, s * (1 + g * (1 - s))
    cdf = 0.5 * (1 + torch.erf(g * (1 / math.sqrt(2))))
    pdf = torch.exp(-0.5 * g * g) * (1 / math.sqrt(2 * math.pi))
    return g * cdf, cdf + g * pdf


class GatedLinear(Op):
    op_type = OperatorType.OP_GATED_LINEAR
    name_prefix = "GatedDense"

    def __init__(self, model, input, out_dim, activation="silu", kernel_initializer=None, name=None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"gated_dense: activation {activation!r}; 'silu' (SwiGLU) or 'gelu' (GeGLU) expected")
        super().__init__(model, [input], name)
        self.in_dim = int(input.dims[-1])
        self.out_dim = int(out_dim)
        self.activation = activation
        if self.name is None:
            self.name = self.auto_name(str(out_dim))
        base = kernel_initializer or GlorotUniformInitializer(model._next_seed() if model else 0)
        self._add_weight((2 * self.out_dim, self.in_dim), HalfRowsInitializer(base), "kernel")
        self._finish([tuple(input.dims[:-1]) + (self.out_dim,)])

    def splittable_dims(self):
        return set(range(self.out_ndims - 1))

    def check_hip(self):
        """What neither GPU form can run, raised at compile(): a forced fused form on a shape the fused kernel
        refuses (the launchers also refuse misaligned operands), and widths past the kernels' 32-bit columns."""
        F, H = self.out_dim, self.in_dim
        if 2 * F >= 2 ** 31 or H >= 2 ** 31:
            raise ValueError(f"GatedLinear '{self.name}': {H} -> 2 x {F} features exceed the kernels' 32-bit columns")
        if FORM == "fused" and (F % 4 or H % 8):
            raise ValueError(f"GatedLinear '{self.name}': the fused kernel needs out_dim % 4 == 0 and in_dim % 8 == 0, "
                             f"got {H} -> {F}; FORM 'auto' or 'composed' runs it")

    @staticmethod
    def _buf(ctx, key, rows, cols, like):
        b = ctx.saved.get(key)
        if b is None or b.shape != (rows, cols) or b.dtype != like.dtype or b.device != like.device:
            b = ctx.saved[key] = torch.empty((rows, cols), dtype=like.dtype, device=like.device)
        return b

    def forward(self, ctx: OpCtx):
        x, y = ctx.inputs[0], ctx.outputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        h2 = y.view(-1, y.shape[-1])
        w = ctx.wcompute[0]
        M, H, F = x2.shape[0], self.in_dim, self.out_dim
        gu = self._buf(ctx, "gu", M, 2 * F, h2)
        act = ACTIVATIONS[self.activation]
        if ctx.hip:
            form = FORM
            if form == "auto":
                bf16 = x2.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
                form = AUTO_BF16 if bf16 and K.glu_gemm_eligible(x2, w, gu, h2) else "composed"
            if form == "fused":
                K.glu_gemm_fwd(x2, w, gu, h2, act)
            else:
                K.gemm(x2, x2.stride(0), True, w, H, True, gu, 2 * F, M, 2 * F, H)
                K.glu_act_fwd(gu, h2, act)
            return
        gu.copy_(x2.float() @ w.float().t())
        guf = gu.float()
        h2.copy_(glu_act_torch(guf[:, :F], self.activation)[0] * guf[:, F:])

    def backward(self, ctx: OpCtx, phase="all"):
        """Phases as :meth:`Linear.backward`.  The element-wise pass over (dh, gu) belongs to "dx" (or "all"); a
        "dw" phase that was not preceded by a "dx" runs it itself."""
        x = ctx.inputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        dh2 = ctx.out_grads[0].view(-1, self.out_dim)
        dx = ctx.in_grads[0] if ctx.in_grads else None
        dx2 = None if dx is None else dx.view(-1, dx.shape[-1])
        dw = ctx.weight_grads[0]
        w = ctx.wcompute[0]
        M, H, F = x2.shape[0], self.in_dim, self.out_dim
        gu = ctx.saved["gu"]
        dgu = self._buf(ctx, "dgu", M, 2 * F, gu)
        if phase != "dw" or not ctx.saved.pop("dgu_ready", False):
            if ctx.hip:
                K.glu_act_bwd(dh2, gu, dgu, ACTIVATIONS[self.activation])
            else:
                guf, dhf = gu.float(), dh2.float()
                a, da = glu_act_torch(guf[:, :F], self.activation)
                dgu[:, :F].copy_(dhf * guf[:, F:] * da)
                dgu[:, F:].copy_(dhf * a)
            if phase == "dx":
                ctx.saved["dgu_ready"] = True
        if ctx.hip:
            if dx2 is not None and phase != "dw":
                K.gemm(dgu, 2 * F, True, w, H, False, dx2, dx2.stride(0), M, H, 2 * F, beta=bool(ctx.in_grad_accumulate[0]))
            if phase != "dx":
                K.gemm(dgu, 2 * F, False, x2, x2.stride(0), False, dw, H, 2 * F, H, M, beta=True)
            return
        if phase != "dx":
            dw.add_(dgu.float().t() @ x2.float())
        if dx2 is not None and phase != "dw":
            store(dx2, dgu.float() @ w.float(), ctx.in_grad_accumulate[0])

    def flops(self, in_shapes, out_shapes):
        b = 1
        for d in out_shapes[0][:-1]:
            b *= d
        return 2.0 * b * in_shapes[0][-1] * 2 * out_shapes[0][-1]
