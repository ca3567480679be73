"""Rotary position embeddings in the Attention op on the fp32 CPU executor: forward and written-out backward
against float64 autograd of the explicit formula, the builder against the same composition in torch, the two
refusals, and a world-2 sample split (the table depends on the position only)."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_attention_cpu import _cpu_model

BASE = 10000.0


def rotate_f64(x, base, interleaved, transpose=False):
    """x float64 [..., T, dh]: row t rotated by the angles t * base ** (-2 i / dh) (``transpose``: by their negatives)."""
    T, dh = x.shape[-2:]
    ang = torch.arange(T, dtype=torch.float64, device=x.device)[:, None] * \
        base ** (-torch.arange(0, dh, 2, dtype=torch.float64, device=x.device) / dh)
    c, s = ang.cos(), -ang.sin() if transpose else ang.sin()
    lo, hi = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :dh // 2], x[..., dh // 2:])
    lo, hi = lo * c - hi * s, hi * c + lo * s
    return torch.stack((lo, hi), -1).flatten(-2) if interleaved else torch.cat((lo, hi), -1)


def rope_attention_f64(q, k, v, H, KH, causal, lengths, inter):
    B, Tq, Tk, dh = q.shape[0], q.shape[1], k.shape[1], q.shape[2] // H
    sp = lambda t, n: t.double().reshape(B, t.shape[1], n, dh).transpose(1, 2)   # noqa: E731
    qr, kr = rotate_f64(sp(q, H), BASE, inter), rotate_f64(sp(k, KH), BASE, inter).repeat_interleave(H // KH, 1)
    vis = torch.ones(Tq, Tk, dtype=torch.bool)
    vis = (vis.tril() if causal else vis)[None, None]
    if lengths is not None:
        vis = vis & (torch.arange(Tk)[None, :] < torch.tensor(lengths)[:, None])[:, None, None, :]
    s = (qr @ kr.transpose(-1, -2) * dh ** -0.5).masked_fill(~vis, float("-inf"))
    return (torch.softmax(s, -1) @ sp(v, KH).repeat_interleave(H // KH, 1)).transpose(1, 2).reshape(B, Tq, H * dh)


@pytest.mark.parametrize("inter", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("H,KH,Tq,Tk,causal,lengths", [(4, 2, 7, 7, True, [7, 3]), (2, 2, 5, 9, False, None)],
                         ids=["causal-gqa-lengths", "cross"])
def test_rope_op_matches_autograd(H, KH, Tq, Tk, causal, lengths, inter):
    from flexmi.core.types import DataType
    from flexmi.ops.base import OpCtx
    B, dh = 2, 6
    m = _cpu_model(B)
    len_t = None if lengths is None else m.create_tensor([B, 1], DataType.DT_INT32)
    op = m.attention(*(m.create_tensor([B, T, n * dh]) for T, n in ((Tq, H), (Tk, KH), (Tk, KH))), H, causal, kv_heads=KH,
                     key_lengths=len_t, rope_base=BASE, rope_interleaved=inter).owner_op
    g = torch.Generator().manual_seed(4)
    vals = [torch.randn(B, T, n * dh, generator=g, requires_grad=True) for T, n in ((Tq, H), (Tk, KH), (Tk, KH))]
    dy = torch.randn(B, Tq, H * dh, generator=g)
    ref = rope_attention_f64(*vals, H, KH, causal, lengths, inter)
    ref.backward(dy.double())
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs = [x.detach().clone() for x in vals] + ([] if lengths is None else [torch.tensor(lengths, dtype=torch.int32)[:, None]])
    ctx.outputs = [torch.full((B, Tq, H * dh), float("nan"))]
    op.forward(ctx)
    torch.testing.assert_close(ctx.outputs[0], ref.detach().float(), rtol=0, atol=1e-5)
    prev = [torch.randn_like(x) for x in vals]
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate = [dy.clone()], [p.clone() for p in prev], [True, False, True]
    op.backward(ctx)
    for i, (got, p, x) in enumerate(zip(ctx.in_grads, prev, vals)):
        torch.testing.assert_close(got, x.grad + (p if i != 1 else 0), rtol=0, atol=1e-5, msg=f"input {i}")


def test_rope_multihead_attention_is_the_composition():
    from flexmi.core import LossType, SGDOptimizer
    B, T, E, H, KH = 3, 6, 16, 4, 2
    m = _cpu_model(B)
    x = m.create_tensor([B, T, E])
    out = m.multihead_attention(x, x, x, E, H, causal=True, name="mha", num_kv_heads=KH, rope_base=BASE)
    m.compile(SGDOptimizer(m, 0.0), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    wq, bq, wk, bk, wv, bv, wo, bo = (torch.from_numpy(p.get_weights(m).copy()) for p in m.parameters)
    xv = torch.randn(B, T, E, generator=torch.Generator().manual_seed(6))
    ex.scatter_from_host(x, xv.numpy())
    ex.forward()
    ref = rope_attention_f64(xv @ wq.T + bq, xv @ wk.T + bk, xv @ wv.T + bv, H, KH, True, None, False).float() @ wo.T + bo
    np.testing.assert_allclose(ex.gather_to_host(out), ref.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("E,base,msg", [(6, BASE, "even head dimension"), (8, 0.0, "must be positive")])
def test_rope_refusals(E, base, msg):
    m = _cpu_model(2)
    with pytest.raises(ValueError, match=msg):
        m.attention(*(m.create_tensor([2, 4, E]) for _ in range(3)), 2, rope_base=base)     # dh = E / 2


def _job(rank, world, out):
    """3 SGD steps of a causal rotary encoder layer, every op split on the samples over `world` ranks."""
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    from flexmi.parallel.layout import ParallelConfig
    B, T, E = 8, 6, 16
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, 5
    m = FFModel(cfg)
    x = m.create_tensor([B, T, E])
    m.dense(m.transformer_encoder_layer(x, 4, 32, causal=True, name="enc", num_kv_heads=2, rope_base=BASE,
                                        rope_interleaved=True), 1)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    m.strategies = {op.name: ParallelConfig.data_parallel(op.out_ndims, world) for op in m.layers}
    ex = m.init_layers()
    rng = np.random.RandomState(3)
    for _ in range(3):
        ex.scatter_from_host(x, rng.randn(B, T, E).astype(np.float32))
        ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, T, 1).astype(np.float32))
        ex.train_step()
    params = [p.get_weights(m) for p in m.parameters]
    if rank == 0:
        np.savez(out, *params)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _job(rank, world, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.multiproc
def test_rope_world2_equals_world1():
    res = []
    for world in (1, 2):
        out = tempfile.mktemp(suffix=".npz")
        if world == 1:
            _job(0, 1, out)
        else:
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            mp.start_processes(_worker, args=(world, port, out), nprocs=world, join=True, start_method="spawn")
        d = np.load(out)
        res.append([d[f"arr_{i}"] for i in range(len(d.files))])
        os.unlink(out)
    for a, b in zip(res[1], res[0]):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
