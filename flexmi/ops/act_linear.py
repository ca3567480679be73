"""Dense layer with GELU, tanh-GELU or SiLU (``OP_LINEAR_ACT``), built by ``FFModel.dense(..., activation=
AC_MODE_GELU / AC_MODE_GELU_TANH / AC_MODE_SILU)``.

On ``x [..., H]`` the op returns ``y [..., F]``::

    z = x W^T + b         "pre", kept for the backward
    y = act(z)            exact (erf) GELU ``z Phi(z)``, tanh GELU ``z (1 + tanh(sqrt(2/pi) (z + 0.044715 z^3))) / 2``
                          (torch's ``approximate="tanh"``, GPT-2's) or SiLU ``z sigmoid(z)``

Weights, initialisers, layouts, split dims, names and checkpoint keys are :class:`Linear`'s (fp32 masters ``weight
[F, H]`` and the optional ``bias [F]``), so a model can switch the activation and keep its checkpoints and strategy
files.  What changes is the backward: :class:`Linear` recomputes ``act'`` from the layer's OUTPUT, and none of these
three activations is monotonic, so ``act'`` is no function of the output.  This op keeps the pre-activation instead.
It has its own type, so the executor's Linear-only paths (fuse-below, fused SGD, grouped and deferred dW, the
pipelined tail) do not apply.

Backward is the true gradient: ``dz = dy * act'(z)``, ``db += sum_rows dz``, ``dX (+)= dz W``, ``dW += dz^T x`` with
``silu'(z) = s (1 + z (1 - s))``, ``gelu'(z) = Phi(z) + z phi(z)`` and, for the tanh form with ``t`` the tanh above,
``(1 + t) / 2 + z (1 - t^2) sqrt(2/pi) (1 + 3 * 0.044715 z^2) / 2``.

Rounding rule (both backends, both GPU forms; the rule of :class:`flexmi.ops.gated.GatedLinear`): ``z`` is rounded to
the compute dtype ONCE and kept as ``pre [M, F]`` in ``ctx.saved`` (an op-private buffer allocated in the first
forward and reused, so a captured step replays on one address); ``y`` is computed in fp32 from the stored ``z`` and
rounded once, and the backward reads the same stored ``z``, so the gradient is that of the function the forward
evaluated.  In fp32 nothing is rounded.

On MI355X (``csrc/kernels/act_gemm.hip``) the forward has two forms.  "fused": one MFMA kernel adds the bias, stores
``pre`` and evaluates the activation in its epilogue (bf16; ``F % 4 == 0``, ``H % 8 == 0``, 16-byte aligned rows).
"composed": the Linear forward (GEMM with its bias epilogue) into ``pre``, then the unary kernel (codes 5-7 of
``flexmi/ops/elementwise.py``) from ``pre`` into ``y`` (fp32, and every shape the fused kernel refuses).
:data:`FORM` forces one; "auto" picks per call (see ``profiles/act_linear.txt`` for the measurement behind the
choice).  The backward is ``fm_act_bwd`` writing ``dz`` into an op-private ``dpre [M, F]`` and adding the bias
gradient without atomics (bit-identical from run to run), then Linear's own dX and weight-gradient GEMMs on
``dpre``.  The CPU path is one fp32 ``matmul`` and the formulas above written out.
"""
from __future__ import annotations

import torch

from flexmi.core.types import ActiMode, OperatorType

from . import _kernels as K
from .base import OpCtx, store
from .elementwise import actz_torch
from .linear import Linear

# ActiMode -> the kernels' activation code (the unary codes of flexmi/ops/elementwise.py)
ACT_CODES = {ActiMode.AC_MODE_GELU: 5, ActiMode.AC_MODE_GELU_TANH: 6, ActiMode.AC_MODE_SILU: 7}
# forward form on the HIP backend: "auto" | "fused" | "composed" (tests run both on one shape)
FORM = "auto"
# what "auto" picks for bf16 operands the fused kernel takes (measured: profiles/act_linear.txt)
AUTO_BF16 = "fused"


class ActLinear(Linear):
    op_type = OperatorType.OP_LINEAR_ACT
    checkpoint_name = "Linear"      # parameter keys of flexmi/runtime/checkpoint.py: the same as Linear's

    def __init__(self, model, input, out_dim, activation, *args, **kw):
        if ActiMode(activation) not in ACT_CODES:
            raise ValueError(f"ActLinear: activation {activation!r}; AC_MODE_GELU, AC_MODE_GELU_TANH or AC_MODE_SILU expected")
        super().__init__(model, input, out_dim, activation, *args, **kw)
        self.code = ACT_CODES[self.activation]

    def check_hip(self):
        """What neither GPU form can run, raised at compile(): a forced fused form on a shape the fused kernel
        refuses (the launchers also refuse misaligned operands), and widths past the kernels' 32-bit columns."""
        F, H = self.out_dim, self.in_dim
        if F >= 2 ** 30 or H >= 2 ** 31:
            raise ValueError(f"ActLinear '{self.name}': {H} -> {F} features exceed the kernels' 32-bit columns")
        if FORM == "fused" and (F % 4 or H % 8):
            raise ValueError(f"ActLinear '{self.name}': the fused kernel needs out_dim % 4 == 0 and in_dim % 8 == 0, "
                             f"got {H} -> {F}; FORM 'auto' or 'composed' runs it")

    @staticmethod
    def _buf(ctx, key, like):
        b = ctx.saved.get(key)
        if b is None or b.shape != like.shape or b.dtype != like.dtype or b.device != like.device:
            b = ctx.saved[key] = torch.empty(like.shape, dtype=like.dtype, device=like.device)
        return b

    def forward(self, ctx: OpCtx):
        x, y = ctx.inputs[0], ctx.outputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        y2 = y.view(-1, y.shape[-1])
        w = ctx.wcompute[0]
        b = ctx.weights[1] if self.use_bias else None
        pre = self._buf(ctx, "pre", y2)
        if ctx.hip:
            form = FORM
            if form == "auto":
                bf16 = x2.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
                form = AUTO_BF16 if bf16 and K.act_gemm_eligible(x2, w, b, pre, y2) else "composed"
            if form == "fused":
                K.act_gemm_fwd(x2, w, b, pre, y2, self.code)
            else:
                K.linear_forward(x2, w, b, int(ActiMode.AC_MODE_NONE), pre)
                K.unary_forward(self.code, pre, y2)
            return
        pre.copy_(torch.nn.functional.linear(x2.float(), w.float(), None if b is None else b.float()))
        y2.copy_(actz_torch(self.code, pre.float())[0])

    def backward(self, ctx: OpCtx, phase="all", collect=None):
        """Phases as :meth:`Linear.backward`.  The element-wise pass over (dy, pre) belongs to "dx" (or "all") and
        adds the bias gradient there; a "dw" phase that was not preceded by a "dx" runs it itself."""
        assert collect is None, "ActLinear takes no part in the grouped weight-gradient launch"
        x = ctx.inputs[0]
        x2 = x.reshape(-1, x.shape[-1])
        dy2 = ctx.out_grads[0].view(-1, self.out_dim)
        dx = ctx.in_grads[0] if ctx.in_grads else None
        dx2 = None if dx is None else dx.view(-1, dx.shape[-1])
        dw = ctx.weight_grads[0]
        db = ctx.weight_grads[1] if self.use_bias else None
        w = ctx.wcompute[0]
        pre = ctx.saved["pre"]
        dpre = self._buf(ctx, "dpre", pre)
        if phase != "dw" or not ctx.saved.pop("dpre_ready", False):
            if ctx.hip:
                K.act_bwd(dy2, pre, dpre, db, self.code)
            else:
                dz = dy2.float() * actz_torch(self.code, pre.float())[1]
                dpre.copy_(dz)
                if db is not None:
                    db.add_(dz.sum(0))
            if phase == "dx":
                ctx.saved["dpre_ready"] = True
        acc = bool(ctx.in_grad_accumulate[0]) if dx2 is not None else False
        if ctx.hip:
            # Linear's dX and dW GEMMs of an activation-free layer whose incoming gradient is dpre (db is done)
            K.linear_backward(x2, w, dpre, dpre, int(ActiMode.AC_MODE_NONE), dx2, acc, dw, None, ctx.workspace, False, None,
                              phase, None)
            return
        if phase != "dx":
            dw.add_(dpre.float().t() @ x2.float())
        if dx2 is not None and phase != "dw":
            store(dx2, dpre.float() @ w.float(), acc)
