"""Element-wise unary / binary ops.

Reference: ``src/ops/element_unary.cu`` (cuDNN activations + custom ``exp`` kernel, ``:283-302``,
``:384-404``) and ``src/ops/element_binary.cu`` (cuDNN OpTensor ADD/MUL, SUB via α=-1, DIV
asserts -- caveat C9).  MI355X: vectorised HIP kernels ``csrc/kernels/elementwise.hip`` for all
of relu/sigmoid/tanh/elu/exp and add/sub/mul/div (DIV works).  Any dim may be split.
GELU (exact and tanh form) and SiLU are flexmi extensions (``OP_GELU`` / ``OP_GELU_TANH`` / ``OP_SILU``, unary
codes 5-7; ``csrc/kernels/act_math.h``): their gradient is taken from the op's input.
"""
from __future__ import annotations

import math

import torch

from flexmi.core.types import OperatorType
from flexmi.parallel.layout import Layout

from .base import Op, OpCtx, store
from .gated import glu_act_torch
from . import _kernels as K

UNARY_CODES = {OperatorType.OP_RELU: 0, OperatorType.OP_SIGMOID: 1, OperatorType.OP_TANH: 2,
               OperatorType.OP_ELU: 3, OperatorType.OP_EXP: 4,
               OperatorType.OP_GELU: 5, OperatorType.OP_GELU_TANH: 6, OperatorType.OP_SILU: 7}
BINARY_CODES = {OperatorType.OP_EW_ADD: 0, OperatorType.OP_EW_SUB: 1, OperatorType.OP_EW_MUL: 2,
                OperatorType.OP_EW_DIV: 3}
_UNARY_NAMES = {OperatorType.OP_RELU: "Relu", OperatorType.OP_SIGMOID: "Sigmoid",
                OperatorType.OP_TANH: "Tanh", OperatorType.OP_ELU: "Elu", OperatorType.OP_EXP: "Exp",
                OperatorType.OP_GELU: "Gelu", OperatorType.OP_GELU_TANH: "GeluTanh", OperatorType.OP_SILU: "Silu"}
_BINARY_NAMES = {OperatorType.OP_EW_ADD: "Add", OperatorType.OP_EW_SUB: "Sub",
                 OperatorType.OP_EW_MUL: "Mul", OperatorType.OP_EW_DIV: "Div"}


def actz_torch(code, z):
    """fp32 ``act(z)`` and ``act'(z)`` of the codes 5 (exact GELU), 6 (tanh GELU) and 7 (SiLU), written out (no
    autograd): none of them is monotonic, so the derivative is a function of the input, not of the output"""
    if code == 6:
        k = math.sqrt(2 / math.pi)
        t = torch.tanh(k * (z + 0.044715 * z ** 3))
        return 0.5 * z * (1 + t), 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * k * (1 + 3 * 0.044715 * z * z)
    return glu_act_torch(z, "silu" if code == 7 else "gelu")


def unary_fwd_torch(code, x):
    if code == 0:
        return torch.relu(x)
    if code == 1:
        return torch.sigmoid(x)
    if code == 2:
        return torch.tanh(x)
    if code == 3:
        return torch.nn.functional.elu(x)
    if code >= 5:
        return actz_torch(code, x)[0]
    return torch.exp(x)


def unary_bwd_torch(code, x, y, dy):
    if code == 0:
        return dy * (x > 0).to(dy.dtype)
    if code == 1:
        return dy * y * (1 - y)
    if code == 2:
        return dy * (1 - y * y)
    if code == 3:
        return dy * torch.where(x > 0, torch.ones_like(x), y + 1)
    if code >= 5:
        return dy * actz_torch(code, x)[1]
    return dy * y


class ElementUnary(Op):
    def __init__(self, model, op_type, input, name=None):
        super().__init__(model, [input], name)
        self.op_type = OperatorType(op_type)
        self.code = UNARY_CODES[self.op_type]
        self.name_prefix = _UNARY_NAMES[self.op_type]
        if self.name is None:
            self.name = self.auto_name("")
        self._finish([input.dims])

    def splittable_dims(self):
        return set(range(self.out_ndims))

    def forward(self, ctx: OpCtx):
        if ctx.saved.get("fused_into_binary"):   # the producing ElementBinary wrote relu(a op b) here
            return
        x, y = ctx.inputs[0], ctx.outputs[0]
        if ctx.hip:
            K.unary_forward(self.code, x, y)
        else:
            y.copy_(unary_fwd_torch(self.code, x.float()))

    def backward(self, ctx: OpCtx):
        if not ctx.in_grads or ctx.in_grads[0] is None or ctx.saved.get("fused_into_binary"):
            return
        x, y, dy, dx = ctx.inputs[0], ctx.outputs[0], ctx.out_grads[0], ctx.in_grads[0]
        if getattr(self, "skip_act_grad", False):   # fused sigmoid + BCE (loss emitted dL/dz)
            if ctx.hip:
                K.copy_or_add(dy, dx, ctx.in_grad_accumulate[0])
            else:
                store(dx, dy, ctx.in_grad_accumulate[0])
            return
        if ctx.hip:
            K.unary_backward(self.code, x, y, dy, dx, ctx.in_grad_accumulate[0])
        else:
            store(dx, unary_bwd_torch(self.code, x.float(), y.float(), dy.float()), ctx.in_grad_accumulate[0])


class ElementBinary(Op):
    def __init__(self, model, op_type, x, y, name=None):
        super().__init__(model, [x, y], name)
        self.op_type = OperatorType(op_type)
        self.code = BINARY_CODES[self.op_type]
        self.name_prefix = _BINARY_NAMES[self.op_type]
        assert tuple(x.dims) == tuple(y.dims), "ElementBinary requires same-shape inputs (reference semantics)"
        if self.name is None:
            self.name = self.auto_name("")
        self._finish([x.dims])

    def splittable_dims(self):
        return set(range(self.out_ndims))

    def forward(self, ctx: OpCtx):
        a, b, y = ctx.inputs[0], ctx.inputs[1], ctx.outputs[0]
        fused = ctx.saved.get("fused_relu")      # (relu output, its gradient): executor fusion
        if ctx.hip and fused is not None:
            K.binary_forward(self.code, a, b, fused[0], relu=True)
            return
        if ctx.hip:
            K.binary_forward(self.code, a, b, y)
        else:
            a, b = a.float(), b.float()
            y.copy_([a + b, a - b, a * b, a / b][self.code])

    def backward(self, ctx: OpCtx):
        a, b, dy = ctx.inputs[0], ctx.inputs[1], ctx.out_grads[0]
        da = ctx.in_grads[0] if len(ctx.in_grads) > 0 else None
        db = ctx.in_grads[1] if len(ctx.in_grads) > 1 else None
        if ctx.hip:
            fused = ctx.saved.get("fused_relu")
            g, ymask = (fused[1], fused[0]) if fused is not None else (dy, None)
            acca, accb = ctx.in_grad_accumulate[0], ctx.in_grad_accumulate[1]
            if da is not None and db is not None and da.data_ptr() == db.data_ptr():
                # op(t, t): both gradients go to t's buffer.  The kernel's outputs are __restrict__,
                # so each gets a launch of its own, the second adding to the first
                K.binary_backward(self.code, a, b, g, da, None, acca, False, ymask=ymask)
                K.binary_backward(self.code, a, b, g, None, db, False, True, ymask=ymask)
                return
            K.binary_backward(self.code, a, b, g, da, db, acca, accb, ymask=ymask)
            return
        a, b, g = a.float(), b.float(), dy.float()
        if self.code == 0:
            ga, gb = g, g
        elif self.code == 1:
            ga, gb = g, -g
        elif self.code == 2:
            ga, gb = g * b, g * a
        else:
            ga, gb = g / b, -g * a / (b * b)
        if da is not None:
            store(da, ga, ctx.in_grad_accumulate[0])
        if db is not None:
            store(db, gb, ctx.in_grad_accumulate[1])
