"""Linear in MXFP8 (``OP_LINEAR_MX``): the three GEMMs of a dense layer on block-scaled fp8.

Weights, layouts, split dims and names are :class:`Linear`'s (fp32 masters; checkpoints and strategy
files are interchangeable).  Only the arithmetic of the products changes (``flexmi/ops/mx.py``):

    forward   y  = act(Xr Wr^T + b)     X, W -> e4m3, blocks of 32 along in_dim
    backward  G  = dy * act'(y)         fp32 -> e5m2, both copies, db += column sums of the fp32 G
              dX = Gr Wc^T              blocks along out_dim
              dW += Gc Xc^T             blocks along the rows (zero-padded to a multiple of 128)

r / c are the row- / column-wise copy of an operand: one quantiser pass writes both, the column-wise one
transposed, so every GEMM is ``A[M, K] B[N, K]^T`` on K-contiguous codes (``csrc/kernels/mxfp8.hip``).
The copies made in the forward stay in ``ctx.saved`` for the backward; weights are re-quantised every
step.  The op has its own type, so the executor's Linear-only paths (fuse-below, fused SGD, grouped and
deferred dW, the pipelined tail) do not apply.  The CPU path does the same quantised arithmetic with
:func:`mx_quantize_torch` and fp32 matmuls.
"""
from __future__ import annotations

import torch

from flexmi.core.types import ActiMode, OperatorType

from . import _kernels as K
from .base import OpCtx, store
from .linear import Linear, act_backward_torch, act_forward_torch
from .mx import FMT_E4M3, FMT_E5M2, mx_quantize_torch, pad128


def mx_eligible(in_dim, out_dim):
    """The widths the MX kernels take: both multiples of the 32-element block."""
    return in_dim % 32 == 0 and out_dim % 32 == 0


def _deq(t, dim, fmt):
    """fp32 values of ``t`` quantised along ``dim``, zero-padded there to a multiple of 128 first"""
    n = t.shape[dim]
    if n % 128:
        pad = list(t.shape)
        pad[dim] = pad128(n) - n
        t = torch.cat([t, t.new_zeros(pad)], dim)
    return mx_quantize_torch(t, dim, fmt)[2].narrow(dim, 0, n)


class LinearMX(Linear):
    op_type = OperatorType.OP_LINEAR_MX
    checkpoint_name = "Linear"      # parameter keys of flexmi/runtime/checkpoint.py: the same as Linear's

    def __init__(self, model, input, out_dim, *args, **kw):
        if not mx_eligible(input.dims[-1], int(out_dim)):
            raise ValueError(f"dense(fp8=True): {input.dims[-1]} -> {out_dim} features; MXFP8 needs both widths to be "
                             f"multiples of 32")
        super().__init__(model, input, out_dim, *args, **kw)

    def check_hip(self):
        """The limits of the HIP kernels (csrc/kernels/mxfp8.hip), raised at compile(); the launchers also
        refuse operands whose rows are not 16-byte aligned."""
        if not mx_eligible(self.in_dim, self.out_dim):
            raise ValueError(f"LinearMX '{self.name}': {self.in_dim} -> {self.out_dim}, both must be multiples of 32")

    @staticmethod
    def _bufs(ctx, key, rows, cols, device):
        b = ctx.saved.get(key)
        if b is None or b[0].shape != (rows, cols):
            b = ctx.saved[key] = K.mx_alloc(rows, cols, device)
        return b

    def forward(self, ctx: OpCtx):
        x = ctx.inputs[0]
        y = ctx.outputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        y2 = y.view(-1, y.shape[-1])
        w = ctx.wcompute[0]
        b = ctx.weights[1] if self.use_bias else None
        if ctx.hip:
            M, Kd, N = x2.shape[0], x2.shape[1], w.shape[0]
            xq = self._bufs(ctx, "mx_x", M, Kd, x.device)
            wq = self._bufs(ctx, "mx_w", N, Kd, x.device)
            K.mx_quant(x2, FMT_E4M3, *xq)
            K.mx_quant(w, FMT_E4M3, *wq)
            K.mx_gemm(xq[0], xq[1], FMT_E4M3, wq[0], wq[1], FMT_E4M3, y2, M, N, Kd, bias=b, act=int(self.activation))
        else:
            out = _deq(x2, 1, "e4m3") @ _deq(w, 1, "e4m3").t()
            if b is not None:
                out = out + b.float()
            y2.copy_(act_forward_torch(out, self.activation))

    def backward(self, ctx: OpCtx, phase="all", collect=None):
        """Phases as :meth:`Linear.backward`.  The quantiser pass over (dy, y) belongs to "dx" (or "all") and adds
        the bias gradient there; a "dw" phase that was not preceded by a "dx" runs it itself."""
        assert collect is None, "LinearMX takes no part in the grouped weight-gradient launch"
        x = ctx.inputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        y2 = ctx.outputs[0].view(-1, ctx.outputs[0].shape[-1])
        dy2 = ctx.out_grads[0].view(y2.shape)
        dx = ctx.in_grads[0] if ctx.in_grads else None
        dx2 = None if dx is None else dx.view(-1, dx.shape[-1])
        dw = ctx.weight_grads[0]
        db = ctx.weight_grads[1] if self.use_bias else None
        act = ActiMode.AC_MODE_NONE if getattr(self, "skip_act_grad", False) else self.activation
        w = ctx.wcompute[0]
        M, Kd, N = x2.shape[0], x2.shape[1], w.shape[0]
        if ctx.hip:
            gq = self._bufs(ctx, "mx_g", M, N, x.device)
            if phase != "dw" or not ctx.saved.pop("mx_g_ready", False):
                K.mx_quant_dact(dy2, y2, int(act), *gq, db)
                if phase == "dx":
                    ctx.saved["mx_g_ready"] = True
            xq, wq = ctx.saved["mx_x"], ctx.saved["mx_w"]
            if dx2 is not None and phase != "dw":
                K.mx_gemm(gq[0], gq[1], FMT_E5M2, wq[2], wq[3], FMT_E4M3, dx2, M, Kd, N,
                          beta=bool(ctx.in_grad_accumulate[0]))
            if phase != "dx":
                K.mx_gemm(gq[2], gq[3], FMT_E5M2, xq[2], xq[3], FMT_E4M3, dw, N, Kd, pad128(M), beta=True)
            return
        dpre = act_backward_torch(dy2.float(), y2.float(), act)
        if phase != "dx":
            dw.add_(_deq(dpre, 0, "e5m2").t() @ _deq(x2, 0, "e4m3"))
            if db is not None:
                db.add_(dpre.sum(0))
        if dx2 is not None and phase != "dw":
            store(dx2, _deq(dpre, 1, "e5m2") @ _deq(w, 0, "e4m3"), ctx.in_grad_accumulate[0])
