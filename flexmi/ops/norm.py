"""LayerNorm and RMSNorm over the last dim with a fused residual add (``OP_LAYERNORM``).

Inputs ``[x]`` or ``[x, residual]`` of one shape ``[..., D]``; ``s = x + residual`` (``s = x`` without
one) is formed in fp32 and never rounded to the storage type.

  LayerNorm: ``y = (s - mean_D s) * rsqrt(var_D s + eps) * gamma + beta`` (biased variance)
  RMSNorm (``rms=True``): ``y = s * rsqrt(mean_D s^2 + eps) * gamma`` -- no mean, no ``beta``

Weights ``scale`` (D,) = 1 and ``bias`` (D,) = 0 are fp32 masters used directly, as in ``BatchNorm``;
``elementwise_affine=False`` creates none.  Rows are independent, so every dim but the last may be
split; the weights are replicated and their gradients take the ordinary bucketed all-reduce.

Backward, with ``xhat`` the normalised ``s``, ``g = dy * gamma`` and ``rstd`` the rsqrt above:
``ds = rstd * (g - mean_D g - xhat * mean_D(g * xhat))`` (RMSNorm: without ``mean_D g``);
``dx (+)= ds`` and ``dresidual (+)= ds``, each with its own accumulate flag.  ``dgamma += sum_R dy *
xhat`` and ``dbeta += sum_R dy`` ADD to the fp32 weight-gradient buffers, as Linear's dW does: the
executor zeroes them before a step's backward starts.

On MI355X ``csrc/kernels/layernorm.hip`` runs it with the row held in registers (``D <= 8192``,
:meth:`LayerNorm.check_hip`); the only state kept for the backward is fp32 (mean, rstd) per row,
allocated once in ``ctx.saved`` so a captured step replays on one address.  The CPU path is the
formulas above in fp32, the backward written out.
"""
from __future__ import annotations

import torch

from flexmi.core.initializers import ConstantInitializer, ZeroInitializer
from flexmi.core.types import OperatorType

from .base import Op, OpCtx, store
from . import _kernels as K


class LayerNorm(Op):
    op_type = OperatorType.OP_LAYERNORM
    name_prefix = "LayerNorm"
    HIP_MAX_D = 8192

    def __init__(self, model, x, residual=None, eps=1e-5, elementwise_affine=True, rms=False, name=None):
        if residual is not None and residual is x:
            raise ValueError("LayerNorm: residual is x -- pass x alone, or scale it first (an op must not receive one "
                             "tensor as two inputs)")
        super().__init__(model, [x] + ([residual] if residual is not None else []), name)
        if len(x.dims) < 1:
            raise ValueError("LayerNorm: x must have at least one dim")
        if residual is not None and tuple(residual.dims) != tuple(x.dims):
            raise ValueError(f"LayerNorm: x {tuple(x.dims)} needs a residual of its shape, got {tuple(residual.dims)}")
        self.D, self.eps, self.affine, self.rms = int(x.dims[-1]), float(eps), bool(elementwise_affine), bool(rms)
        if self.name is None:
            self.name = self.auto_name(str(self.D))
        if self.affine:
            self._add_weight((self.D,), ConstantInitializer(1.0), "scale")
            if not self.rms:
                self._add_weight((self.D,), ZeroInitializer(), "bias")
        self._finish([tuple(x.dims)])

    def check_hip(self):
        """The limit of the HIP kernels (csrc/kernels/layernorm.hip), raised at compile()."""
        if self.D > self.HIP_MAX_D:
            raise ValueError(f"LayerNorm '{self.name}' normalises over {self.D} features: the HIP kernels take at most "
                             f"{self.HIP_MAX_D}; the CPU backend has no limit")

    def splittable_dims(self):
        return set(range(self.out_ndims - 1))

    def _weights(self, ctx):
        gamma = ctx.weights[0] if self.affine else None
        beta = ctx.weights[1] if self.affine and not self.rms else None
        return gamma, beta

    def _xhat(self, ctx):
        """fp32 (xhat, rstd) of the CPU path"""
        s = ctx.inputs[0].float()
        if len(ctx.inputs) > 1:
            s = s + ctx.inputs[1].float()
        if self.rms:
            rstd = torch.rsqrt((s * s).mean(-1, keepdim=True) + self.eps)
            return s * rstd, rstd
        c = s - s.mean(-1, keepdim=True)
        rstd = torch.rsqrt((c * c).mean(-1, keepdim=True) + self.eps)
        return c * rstd, rstd

    def forward(self, ctx: OpCtx):
        x, y = ctx.inputs[0], ctx.outputs[0]
        gamma, beta = self._weights(ctx)
        if ctx.hip:
            rows = x.numel() // self.D
            stats = ctx.saved.get("stats")
            if stats is None or stats.shape[0] != rows:
                stats = ctx.saved["stats"] = torch.empty((rows,) if self.rms else (rows, 2), dtype=torch.float32,
                                                         device=x.device)
            r = ctx.inputs[1].view(-1, self.D) if len(ctx.inputs) > 1 else None
            K.layernorm_forward(x.view(-1, self.D), r, y.view(-1, self.D), gamma, beta, stats, self.eps, self.rms)
            return
        out, _ = self._xhat(ctx)
        if gamma is not None:
            out = out * gamma
        if beta is not None:
            out = out + beta
        y.copy_(out)

    def backward(self, ctx: OpCtx):
        dy = ctx.out_grads[0]
        n = len(ctx.inputs)
        g = (list(ctx.in_grads) + [None, None])[:2]
        acc = (list(ctx.in_grad_accumulate) + [False, False])[:2]
        if n == 1:
            g[1] = None
        gamma, _ = self._weights(ctx)
        dgamma = ctx.weight_grads[0] if self.affine else None
        dbeta = ctx.weight_grads[1] if self.affine and not self.rms else None
        if g[0] is None and g[1] is None and dgamma is None:
            return
        if ctx.hip:
            two = lambda t: None if t is None else t.view(-1, self.D)   # noqa: E731
            K.layernorm_backward(two(ctx.inputs[0]), two(ctx.inputs[1]) if n > 1 else None, two(dy), gamma,
                                 ctx.saved["stats"], two(g[0]), two(g[1]), acc[0], acc[1], dgamma, dbeta, self.rms)
            return
        xhat, rstd = self._xhat(ctx)
        dyf = dy.float()
        if dgamma is not None:
            dgamma.add_((dyf * xhat).reshape(-1, self.D).sum(0))
        if dbeta is not None:
            dbeta.add_(dyf.reshape(-1, self.D).sum(0))
        gg = dyf * gamma if gamma is not None else dyf
        ds = gg - xhat * (gg * xhat).mean(-1, keepdim=True)
        if not self.rms:
            ds = ds - gg.mean(-1, keepdim=True)
        ds = ds * rstd
        for t, a in zip(g, acc):
            if t is not None:
                store(t, ds, a)

    def flops(self, i, o):
        """About 8 flops per element forward; the op is priced by the bytes it moves."""
        n = 1
        for d in i[0]:
            n *= d
        return 8.0 * n
