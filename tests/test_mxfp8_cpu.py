"""MXFP8 on the CPU backend: the builder (``dense(fp8=...)``, ``--linear-fp8``), LinearMX's arithmetic against an
fp64 recomputation from mx_quantize_torch's dequantised tensors, and checkpoint exchange with Linear."""
import os
import tempfile

import numpy as np
import pytest
import torch


def _model(B, argv=None, seed=0):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig(argv)
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, seed
    return FFModel(cfg)


def _deq64(t, dim, fmt):
    """fp64 values of t quantised along dim by mx_quantize_torch (over zero-padded rows, as the op does)"""
    from flexmi.ops.linear_mx import _deq
    return _deq(t, dim, fmt).double()


def test_op_matches_fp64_of_dequantised():
    from flexmi.core.types import ActiMode, OperatorType
    from flexmi.ops.base import OpCtx
    m = _model(70)
    op = m.dense(m.create_tensor([70, 96]), 64, ActiMode.AC_MODE_RELU, fp8=True).owner_op
    assert int(op.op_type) == 107 and op.op_type == OperatorType.OP_LINEAR_MX and op.name.startswith("Dense")
    g = torch.Generator().manual_seed(1)
    x, w, b, dy, dx0, dw0, db0 = (torch.randn(s, generator=g) for s in ((70, 96), (64, 96), (64,), (70, 64), (70, 96), (64, 96), (64,)))
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs, ctx.weights, ctx.wcompute, ctx.outputs = [x], [w, b], [w], [torch.empty(70, 64)]
    op.forward(ctx)
    y = torch.relu(_deq64(x, 1, "e4m3") @ _deq64(w, 1, "e4m3").t() + b.double())
    torch.testing.assert_close(ctx.outputs[0].double(), y, rtol=0, atol=1e-5 * y.abs().max().item())
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate = [dy], [dx0.clone()], [True]
    ctx.weight_grads = [dw0.clone(), db0.clone()]
    op.backward(ctx)
    dpre = dy * (ctx.outputs[0] > 0)
    want = (dx0.double() + _deq64(dpre, 1, "e5m2") @ _deq64(w, 0, "e4m3"),
            dw0.double() + _deq64(dpre, 0, "e5m2").t() @ _deq64(x, 0, "e4m3"), db0.double() + dpre.double().sum(0))
    for got, ref in zip((ctx.in_grads[0], *ctx.weight_grads), want):
        torch.testing.assert_close(got.double(), ref, rtol=0, atol=1e-5 * ref.abs().max().item())


def test_builder_rules():
    from flexmi.core.types import OperatorType
    m = _model(8)
    with pytest.raises(ValueError, match="multiples of 32"):
        m.dense(m.create_tensor([8, 40]), 64, fp8=True)
    m = _model(8, ["prog", "--linear-fp8"])
    h = m.dense(m.create_tensor([8, 13]), 512)
    out = m.dense(h, 256)
    assert h.owner_op.op_type == OperatorType.OP_LINEAR and out.owner_op.op_type == OperatorType.OP_LINEAR_MX
    assert m.dense(out, 32, fp8=False).owner_op.op_type == OperatorType.OP_LINEAR


def test_linear_checkpoint_loads_into_linear_mx():
    from flexmi.core import LossType, SGDOptimizer

    def build(fp8):
        m = _model(8, seed=3 + int(fp8))                               # different initial weights on purpose
        m.dense(m.dense(m.create_tensor([8, 64]), 32, fp8=fp8), 32, fp8=fp8)
        m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
        m.init_layers()
        return m

    src, dst, path = build(False), build(True), os.path.join(tempfile.mkdtemp(), "ck")
    src.save_checkpoint(path)
    dst.load_checkpoint(path)
    for a, b in zip(src.parameters, dst.parameters):
        assert np.array_equal(a.get_weights(src), b.get_weights(dst))
