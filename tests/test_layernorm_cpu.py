"""The LayerNorm op against float64 autograd and ``FFModel.transformer_encoder_layer`` against
``torch.nn.TransformerEncoderLayer`` (weights copied by the documented mapping) on the fp32 CPU executor."""
import numpy as np
import pytest
import torch


def _cpu_model(B):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    return FFModel(cfg)


def norm_f64(x, r, gamma, beta, eps, rms):
    """float64 LayerNorm (torch's) or the written-out RMS formula of x (+ r) over the last dim."""
    s = x.double() + (r.double() if r is not None else 0)
    if rms:
        y = s * torch.rsqrt((s * s).mean(-1, keepdim=True) + eps)
        return y * gamma.double() if gamma is not None else y
    return torch.nn.functional.layer_norm(s, s.shape[-1:], None if gamma is None else gamma.double(),
                                          None if beta is None else beta.double(), eps)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("residual", [False, True], ids=["x", "x+r"])
def test_op_matches_autograd(residual, rms, affine):
    from flexmi.ops.base import OpCtx
    shape = [4, 6, 10]
    m = _cpu_model(4)
    x = m.create_tensor(shape)
    out = m.layer_norm(x, m.create_tensor(shape) if residual else None, 1e-5, affine, rms)
    op = out.owner_op
    nw = (1 if rms else 2) if affine else 0
    assert tuple(out.dims) == tuple(shape) and op.splittable_dims() == {0, 1} and len(op.weights) == nw
    g = torch.Generator().manual_seed(4)
    ins = [torch.randn(shape, generator=g, requires_grad=True) for _ in range(2 if residual else 1)]
    ws = [torch.randn(10, generator=g, requires_grad=True) for _ in range(nw)]
    dy = torch.randn(shape, generator=g)
    ref = norm_f64(ins[0], ins[1] if residual else None, *(ws + [None, None])[:2], 1e-5, rms)
    ref.backward(dy.double())

    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs = [t.detach().clone() for t in ins]
    ctx.weights = [w.detach().clone() for w in ws]
    ctx.outputs = [torch.full(shape, float("nan"))]
    op.forward(ctx)
    torch.testing.assert_close(ctx.outputs[0], ref.detach().float(), rtol=0, atol=1e-5)
    prev = [torch.randn(shape, generator=g) for _ in ins]
    wprev = [torch.randn(10, generator=g) for _ in ws]
    ctx.out_grads = [dy.clone()]
    ctx.in_grads = [p.clone() for p in prev]
    ctx.in_grad_accumulate = [True, False][:len(ins)]
    ctx.weight_grads = [p.clone() for p in wprev]
    op.backward(ctx)
    for got, p, t, a in zip(ctx.in_grads, prev, ins, ctx.in_grad_accumulate):
        torch.testing.assert_close(got, t.grad + (p if a else 0), rtol=0, atol=1e-5)
    for got, p, w in zip(ctx.weight_grads, wprev, ws):                 # weight gradients add to what is there
        torch.testing.assert_close(got, w.grad + p, rtol=0, atol=2e-5)


def test_residual_is_x_is_refused():
    m = _cpu_model(2)
    x = m.create_tensor([2, 8])
    with pytest.raises(ValueError, match="residual is x"):
        m.layer_norm(x, residual=x)


@pytest.mark.parametrize("norm_first", [False, True], ids=["post", "pre"])
def test_encoder_layer_matches_torch(norm_first):
    from flexmi.core import LossType, SGDOptimizer
    from flexmi.core.types import OperatorType
    B, T, E, H, FF = 4, 6, 16, 4, 24
    m = _cpu_model(B)
    x = m.create_tensor([B, T, E])
    enc = m.transformer_encoder_layer(x, H, FF, causal=True, norm_first=norm_first, name="enc")
    m.dense(enc, 1, name="head")
    assert [sum(op.op_type == t for op in m.layers) for t in (OperatorType.OP_LAYERNORM, OperatorType.OP_EW_ADD)] == [2, 2 * norm_first]
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(2)
    for p in m.parameters:                               # norm weights away from (1, 0), so their mapping is tested
        if "norm" in p.name:
            p.set_weights(m, rng.randn(E).astype(np.float32))
    ref = torch.nn.TransformerEncoderLayer(E, H, FF, dropout=0.0, batch_first=True, norm_first=norm_first)
    head = torch.nn.Linear(E, 1)
    # the mapping of the builder's docstring: parameter name -> (torch parameter, its rows)
    tp = {f"enc_attn_{s}.{k}": (getattr(ref.self_attn, f"in_proj_{k}"), slice(i * E, (i + 1) * E))
          for i, s in enumerate("qkv") for k in ("weight", "bias")}
    for n, mod in {"enc_attn_o": ref.self_attn.out_proj, "enc_ff1": ref.linear1, "enc_ff2": ref.linear2, "head": head}.items():
        tp.update({n + ".weight": (mod.weight, slice(None)), n + ".bias": (mod.bias, slice(None))})
    for n, mod in {"enc_norm1": ref.norm1, "enc_norm2": ref.norm2}.items():
        tp.update({n + ".scale": (mod.weight, slice(None)), n + ".bias": (mod.bias, slice(None))})
    assert set(tp) == {p.name for p in m.parameters}
    with torch.no_grad():
        for p in m.parameters:
            tp[p.name][0][tp[p.name][1]].copy_(torch.from_numpy(p.get_weights(m).copy()))
    xv, lab = rng.randn(B, T, E).astype(np.float32), rng.randn(B, T, 1).astype(np.float32)
    ex.scatter_from_host(x, xv)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    ex.forward()
    ex.backward()
    out = ref(torch.from_numpy(xv), src_mask=torch.nn.Transformer.generate_square_subsequent_mask(T))
    (0.5 * (head(out) - torch.from_numpy(lab)).pow(2).sum() / B).backward()
    np.testing.assert_allclose(ex.gather_to_host(enc), out.detach().numpy(), rtol=1e-4, atol=1e-5)
    for p in m.parameters:
        want = tp[p.name][0].grad[tp[p.name][1]].numpy()
        np.testing.assert_allclose(ex.wentries[p.guid].grad.reshape(want.shape).numpy(), want, rtol=1e-4, atol=1e-5,
                                   err_msg=p.name)
