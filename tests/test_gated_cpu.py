"""GatedLinear on the fp32 CPU backend against fp64 autograd, the Llama configuration of ``transformer_encoder_layer``
against a torch.nn.functional module, the builder's defaults and refusals, and sample-split training over gloo."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F


def _cpu_model(B, seed=5):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, seed
    return FFModel(cfg)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_op_matches_autograd(act):
    from flexmi.ops.base import OpCtx
    B, T, H, FF = 3, 5, 12, 10
    m = _cpu_model(B)
    op = m.gated_dense(m.create_tensor([B, T, H]), FF, act).owner_op
    g = torch.Generator().manual_seed(1)
    x, w, dh, dx0, dw0 = (torch.randn(s, generator=g) for s in ((B, T, H), (2 * FF, H), (B, T, FF), (B, T, H), (2 * FF, H)))
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs, ctx.weights, ctx.wcompute, ctx.outputs = [x], [w], [w], [torch.empty(B, T, FF)]
    op.forward(ctx)
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate, ctx.weight_grads = [dh], [dx0.clone()], [True], [dw0.clone()]
    op.backward(ctx)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    ref = (F.silu if act == "silu" else F.gelu)(x64 @ w64[:FF].t()) * (x64 @ w64[FF:].t())
    ref.backward(dh.double())
    assert rel_err(ctx.outputs[0], ref.detach()) < 1e-5
    assert rel_err(ctx.in_grads[0], dx0.double() + x64.grad) < 1e-5
    assert rel_err(ctx.weight_grads[0], dw0.double() + w64.grad) < 1e-5


def _llama_ref(x, W, heads, FF):      # by the documented weight mapping; no rotary positions, no mask
    B, T, E = x.shape
    rms = lambda t, g: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + 1e-5) * g      # noqa: E731
    n1 = rms(x, W["l_norm1.scale"])
    q, k, v = (F.linear(n1, W[f"l_attn_{s}.weight"]).view(B, T, heads, -1).transpose(1, 2) for s in "qkv")
    a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, E)
    h = x + F.linear(a, W["l_attn_o.weight"])
    n2 = rms(h, W["l_norm2.scale"])
    gate, up = W["l_ff1.kernel"][:FF], W["l_ff1.kernel"][FF:]
    return h + F.linear(F.silu(F.linear(n2, gate)) * F.linear(n2, up), W["l_ff2.weight"])


def test_llama_layer_matches_torch():
    from flexmi.core import LossType, SGDOptimizer
    B, T, E, heads, FF = 4, 6, 16, 4, 24
    m = _cpu_model(B)
    x = m.create_tensor([B, T, E])
    enc = m.transformer_encoder_layer(x, heads, FF, name="l", ffn="swiglu", rms_norm=True, norm_first=True, ffn_bias=False,
                                      attention_bias=False)
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(2)
    for p in m.parameters:
        if "norm" in p.name:
            p.set_weights(m, rng.rand(E).astype(np.float32) + 0.5)
    W = {p.name: torch.from_numpy(p.get_weights(m).copy()).requires_grad_() for p in m.parameters}
    assert W["l_ff1.kernel"].shape == (2 * FF, E) and len(W) == 8
    xv, lab = rng.randn(B, T, E).astype(np.float32), rng.randn(B, T, E).astype(np.float32)
    ex.scatter_from_host(x, xv)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    ex.forward()
    ex.backward()
    out = _llama_ref(torch.from_numpy(xv), W, heads, FF)
    (0.5 * (out - torch.from_numpy(lab)).pow(2).sum() / B).backward()
    np.testing.assert_allclose(ex.gather_to_host(enc), out.detach().numpy(), rtol=1e-4, atol=1e-5)
    kernel = next(p for p in m.parameters if p.name == "l_ff1.kernel")
    np.testing.assert_allclose(ex.wentries[kernel.guid].grad.reshape(2 * FF, E).numpy(), W["l_ff1.kernel"].grad.numpy(),
                               rtol=1e-4, atol=1e-5)


def test_default_layer_is_unchanged():
    m = _cpu_model(2)
    m.transformer_encoder_layer(m.create_tensor([2, 6, 16]), 4, 24, name="enc")
    assert [(op.name, type(op).__name__) for op in m.layers] == [
        ("enc_attn_q", "Linear"), ("enc_attn_k", "Linear"), ("enc_attn_v", "Linear"), ("enc_attn", "Attention"),
        ("enc_attn_o", "Linear"), ("enc_norm1", "LayerNorm"), ("enc_ff1", "Linear"), ("enc_ff2", "Linear"),
        ("enc_norm2", "LayerNorm")]
    assert all(op.use_bias for op in m.layers if type(op).__name__ == "Linear") and not m.layers[5].rms


def test_refusals():
    from flexmi.parallel.layout import ParallelConfig
    m = _cpu_model(2)
    x = m.create_tensor([2, 6, 16])
    with pytest.raises(ValueError, match="activation"):
        m.gated_dense(x, 8, "tanh")
    with pytest.raises(ValueError, match="ffn"):
        m.transformer_encoder_layer(x, 4, 24, ffn="glu")
    op = m.gated_dense(x, 8).owner_op
    assert op.valid_pc(ParallelConfig([1, 2, 1], [0, 1])) and op.valid_pc(ParallelConfig([1, 1, 2], [0, 1]))
    assert not op.valid_pc(ParallelConfig([2, 1, 1], [0, 1])), "the feature dim must not be split"


def _job(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from flexmi.core import LossType, SGDOptimizer
    from flexmi.parallel.layout import ParallelConfig
    B = 32
    m = _cpu_model(B)
    x = m.create_tensor([B, 24])
    y = m.dense(m.gated_dense(x, 40, "gelu"), 8)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    m.strategies = {op.name: ParallelConfig.data_parallel(op.out_ndims, world) for op in m.layers}
    ex = m.init_layers()
    rng = np.random.RandomState(3)
    ex.scatter_from_host(x, rng.randn(B, 24).astype(np.float32))
    ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, 8).astype(np.float32))
    ex.train_step()
    res = [ex.gather_to_host(y)] + [p.get_weights(m) for p in m.parameters]
    if rank == 0:
        np.savez(out, *res)
    if world > 1:
        dist.destroy_process_group()


@pytest.mark.multiproc
def test_world2_equals_world1():
    res = []
    for world in (1, 2):
        out = tempfile.mktemp(suffix=".npz")
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        if world == 1:
            _job(0, 1, port, out)
        else:
            mp.start_processes(_job, args=(world, port, out), nprocs=world, join=True, start_method="spawn")
        d = np.load(out)
        res.append([d[f"arr_{i}"] for i in range(len(d.files))])
        os.unlink(out)
    for a, b in zip(res[1], res[0], strict=True):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5)
