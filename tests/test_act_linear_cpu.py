"""ActLinear (dense with GELU / tanh-GELU / SiLU) and the gelu / silu unary ops on the fp32 CPU backend against fp64
autograd, the ``ffn="gelu"`` encoder layer, and the builder's choices and refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flexmi.core.types import ActiMode

ACTS = {"gelu": (ActiMode.AC_MODE_GELU, F.gelu), "gelu_tanh": (ActiMode.AC_MODE_GELU_TANH, lambda z: F.gelu(z, approximate="tanh")),
        "silu": (ActiMode.AC_MODE_SILU, F.silu)}


def _cpu_model(B, seed=5):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, seed
    return FFModel(cfg)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", list(ACTS))
def test_op_matches_autograd(act, bias, acc):
    from flexmi.ops.act_linear import ActLinear
    from flexmi.ops.base import OpCtx
    B, T, H, FF = 3, 5, 12, 10
    m = _cpu_model(B)
    op = m.dense(m.create_tensor([B, T, H]), FF, ACTS[act][0], bias).owner_op
    assert type(op) is ActLinear and [w.name.split(".")[-1] for w in op.weights] == ["weight", "bias"][:1 + bias]
    g = torch.Generator().manual_seed(1)
    x, w, b, dy, dx0, dw0, db0 = (torch.randn(s, generator=g) for s in ((B, T, H), (FF, H), (FF,), (B, T, FF), (B, T, H),
                                                                         (FF, H), (FF,)))
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs, ctx.weights, ctx.wcompute, ctx.outputs = [x], [w, b][:1 + bias], [w], [torch.empty(B, T, FF)]
    op.forward(ctx)
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate = [dy], [dx0.clone()], [acc]
    ctx.weight_grads = [dw0.clone(), db0.clone()][:1 + bias]
    op.backward(ctx)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    ref = ACTS[act][1](F.linear(x64, w64, b64 if bias else None))
    ref.backward(dy.double())
    assert rel_err(ctx.outputs[0], ref.detach()) < 1e-5
    assert rel_err(ctx.in_grads[0], x64.grad + (dx0.double() if acc else 0)) < 1e-5
    assert rel_err(ctx.weight_grads[0], dw0.double() + w64.grad) < 1e-5
    assert not bias or rel_err(ctx.weight_grads[1], db0.double() + b64.grad) < 1e-5


@pytest.mark.parametrize("act", list(ACTS))
def test_unary_matches_autograd(act):
    from flexmi.ops.base import OpCtx
    m = _cpu_model(4)
    t = m.create_tensor([4, 9])
    op = (m.silu(t) if act == "silu" else m.gelu(t, approximate=act == "gelu_tanh")).owner_op
    g = torch.Generator().manual_seed(2)
    x, dy, dx0 = (torch.randn(4, 9, generator=g) * 2 for _ in range(3))
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs, ctx.outputs = [x], [torch.empty(4, 9)]
    op.forward(ctx)
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate = [dy], [dx0.clone()], [True]
    op.backward(ctx)
    x64 = x.double().requires_grad_()
    ref = ACTS[act][1](x64)
    ref.backward(dy.double())
    assert rel_err(ctx.outputs[0], ref.detach()) < 1e-5
    assert rel_err(ctx.in_grads[0], dx0.double() + x64.grad) < 1e-5


def test_gelu_encoder_layer_trains():
    from flexmi.core import LossType, SGDOptimizer
    B, T, E = 4, 6, 16
    m = _cpu_model(B)
    x = m.create_tensor([B, T, E])
    m.transformer_encoder_layer(x, 4, 24, name="enc", ffn="gelu")
    ops = {op.name: type(op).__name__ for op in m.layers}
    assert ops["enc_ff1"] == "ActLinear" and ops["enc_ff2"] == "Linear"
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(2)
    ex.scatter_from_host(x, rng.randn(B, T, E).astype(np.float32))
    ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, T, E).astype(np.float32))
    before = {p.name: p.get_weights(m).copy() for p in m.parameters}
    ex.train_step()
    after = {p.name: p.get_weights(m) for p in m.parameters}
    assert all(np.isfinite(v).all() for v in after.values())
    assert np.abs(after["enc_ff1.weight"] - before["enc_ff1.weight"]).max() > 0
    assert np.abs(after["enc_ff1.bias"] - before["enc_ff1.bias"]).max() > 0


def test_builder_choices_and_refusals():
    m = _cpu_model(2)
    x = m.create_tensor([2, 6, 32])
    m.transformer_encoder_layer(x, 4, 64, name="r", ffn="relu")
    assert type(next(op for op in m.layers if op.name == "r_ff1")).__name__ == "Linear"
    with pytest.raises(ValueError, match="fp8"):
        m.dense(x, 64, ActiMode.AC_MODE_GELU, fp8=True)
    m.config.linear_fp8 = True
    assert type(m.dense(x, 64, ActiMode.AC_MODE_SILU).owner_op).__name__ == "ActLinear"
    assert type(m.dense(x, 64, ActiMode.AC_MODE_RELU).owner_op).__name__ == "LinearMX"
