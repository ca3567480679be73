"""The combine of a DCNv2 cross layer (Wang et al., "DCN V2", 2021; the interaction of the MLPerf
DLRM-DCNv2 benchmark): ``x_{l+1} = x_0 * (U_l (V_l x_l) + b_l) + x_l``.

The low-rank product ``t = U (V x) + b`` is two ordinary Linear ops (``FFModel.cross_layer``);
:class:`CrossCombine` is the element-wise rest, ``y = x0 * t + x``, one HIP pass per direction
(``csrc/kernels/cross.hip``) where ``multiply`` + ``add`` take two.  No weights, nothing saved
between forward and backward, any dim may be split; it is a row-wise op of the micro-batch
pipelined tail (``Executor._plan_pipeline``).
"""
from __future__ import annotations

from flexmi.core.types import OperatorType

from .base import Op, OpCtx, store
from . import _kernels as K


class CrossCombine(Op):
    """Inputs ``[x0, t, x]`` of one shape: ``y = x0 * t + x``.  Inputs ``[x0, t]``: the first
    layer, whose ``x`` is ``x0`` itself, ``y = x0 * t + x0`` -- the op never takes one tensor as two
    inputs (each input's gradient has its own accumulate flag, decided per input).

    Backward: ``dt = dy * x0``; ``dx0 (+)= dy * t`` (``+ dy`` in the two-input form); ``dx (+)= dy``.
    """
    op_type = OperatorType.OP_CROSS_COMBINE
    name_prefix = "CrossCombine"

    def __init__(self, model, x0, t, x=None, name=None):
        if x is not None and x is x0:
            raise ValueError("CrossCombine: x is x0 -- use the two-input form cross_combine(x0, t) for the first "
                             "cross layer (an op must not receive one tensor as two inputs)")
        if t is x0 or (x is not None and t is x):
            raise ValueError("CrossCombine: t must be a tensor of its own")
        ins = [x0, t] + ([x] if x is not None else [])
        super().__init__(model, ins, name)
        for i in ins[1:]:
            if tuple(i.dims) != tuple(x0.dims):
                raise ValueError(f"CrossCombine: inputs of one shape expected, got {[tuple(i.dims) for i in ins]}")
        self.self_form = x is None
        if self.name is None:
            self.name = self.auto_name("")
        self._finish([x0.dims])

    def splittable_dims(self):
        return set(range(self.out_ndims))

    def forward(self, ctx: OpCtx):
        x0, t, y = ctx.inputs[0], ctx.inputs[1], ctx.outputs[0]
        x = None if self.self_form else ctx.inputs[2]
        if ctx.hip:
            K.cross_forward(x0, t, x, y)
            return
        x0 = x0.float()
        y.copy_(x0 * t.float() + (x0 if x is None else x.float()))

    def backward(self, ctx: OpCtx):
        x0, t, dy = ctx.inputs[0], ctx.inputs[1], ctx.out_grads[0]
        g = list(ctx.in_grads) + [None] * (3 - len(ctx.in_grads))
        acc = list(ctx.in_grad_accumulate) + [False] * (3 - len(ctx.in_grad_accumulate))
        d0, dt, dx = g[0], g[1], (None if self.self_form else g[2])
        if ctx.hip:
            K.cross_backward(dy, x0, t, dt, d0, dx, acc[1], acc[0], acc[2], self.self_form)
            return
        dy = dy.float()
        if dt is not None:
            store(dt, dy * x0.float(), acc[1])
        if d0 is not None:
            v = dy * t.float()
            store(d0, v + dy if self.self_form else v, acc[0])
        if dx is not None:
            store(dx, dy, acc[2])
