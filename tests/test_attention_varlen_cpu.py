"""Attention with per-sample key lengths and grouped-query heads on the CPU executor: the op against a
float64 oracle with NaN in the padded key rows, what compile() refuses, and a gloo world-2 run."""
import functools
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def oracle(q, k, v, dout, heads, kv_heads, causal, lens):
    """float64 output and gradients of a cleaned copy (padded K/V rows zeroed, KV heads repeated):
    e = exp(s - rowmax) * visible, p = e / max(sum e, tiny), so a row without keys gives 0 and no NaN."""
    B, Tq, E = q.shape
    Tk, dh = k.shape[1], E // heads
    live = torch.arange(Tk, device=q.device)[None] < (torch.full((B, 1), Tk, device=q.device) if lens is None else lens)
    vis = live[:, None, None, :] & (torch.ones(Tq, Tk, dtype=torch.bool, device=q.device).tril() if causal else True)
    ins = [q.double().clone().requires_grad_()] + [torch.where(live[:, :, None], t.double(), 0.0).requires_grad_() for t in (k, v)]
    sp = lambda t, n: t.reshape(B, t.shape[1], n, dh).transpose(1, 2)   # noqa: E731
    kh, vh = (sp(t, kv_heads).repeat_interleave(heads // kv_heads, 1) for t in ins[1:])
    s = sp(ins[0], heads) @ kh.transpose(-1, -2) * dh ** -0.5
    e = torch.exp(s - s.amax(-1, keepdim=True).detach()) * vis
    out = (e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(torch.float64).tiny) @ vh).transpose(1, 2).reshape(B, Tq, E)
    out.backward(dout.double())
    return out.detach(), [t.grad for t in ins]


def _model(B, device="cpu"):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = device, "fp32", B, 5
    return FFModel(cfg)


# the first and the last row of the table in tests/test_gpu_attention_varlen.py
@pytest.mark.parametrize("B,H,KH,dh,Tq,Tk,causal,lens,accs", [(4, 2, 2, 32, 33, 70, False, [0, 1, 64, 70], (False, False, False)),
                                                              (2, 4, 2, 128, 130, 130, True, [7, 130], (True, False, True))])
def test_op_matches_float64(B, H, KH, dh, Tq, Tk, causal, lens, accs):
    from flexmi.core.types import DataType
    from flexmi.ops.base import OpCtx
    m = _model(B)
    L = m.create_tensor([B, 1], DataType.DT_INT32)
    op = m.attention(*(m.create_tensor([B, T, n * dh]) for T, n in ((Tq, H), (Tk, KH), (Tk, KH))), H, causal, kv_heads=KH,
                     key_lengths=L).owner_op
    g = torch.Generator().manual_seed(3)
    q, k, v, dout = (torch.randn(B, T, n * dh, generator=g) for T, n in ((Tq, H), (Tk, KH), (Tk, KH), (Tq, H)))
    lt = torch.tensor(lens, dtype=torch.int32).reshape(B, 1)
    ref, dref = oracle(q, k, v, dout, H, KH, causal, lt)
    dead = torch.arange(Tk)[None] >= lt
    k[dead], v[dead] = float("nan"), float("nan")
    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs, ctx.outputs, ctx.out_grads = [q, k, v, lt], [torch.full((B, Tq, H * dh), float("nan"))], [dout]
    op.forward(ctx)
    old = [torch.randn_like(t) for t in (q, k, v)]
    ctx.in_grads, ctx.in_grad_accumulate = [o.clone() for o in old] + [None], list(accs) + [False]
    op.backward(ctx)
    assert rel_err(ctx.outputs[0], ref) < 1e-5 and (0 not in lens or (ctx.outputs[0][lens.index(0)] == 0).all())
    for got, want, o, a in zip(ctx.in_grads, dref, old, accs):      # fp32 sums of <= 130 terms against float64
        assert torch.isfinite(got).all() and rel_err(got, want + (o if a else 0)) < 1e-5
    for i in (1, 2):
        assert torch.equal(ctx.in_grads[i][dead], old[i][dead] if accs[i] else torch.zeros_like(old[i][dead]))


@pytest.mark.parametrize("kw,match", [(dict(kv_heads=3), "does not divide"), (dict(kv_heads=2), "needs k and v"),
                                      (dict(lshape=[2, 2]), "key_lengths"), (dict(ldt="DT_FLOAT"), "key_lengths")])
def test_compile_refuses(kw, match):
    from flexmi.core import LossType, SGDOptimizer
    from flexmi.core.types import DataType
    m = _model(2)
    L = m.create_tensor(kw.get("lshape", [2, 1]), DataType[kw.get("ldt", "DT_INT32")])
    with pytest.raises(ValueError, match=match):
        m.attention(m.create_tensor([2, 5, 32]), m.create_tensor([2, 5, 32]), m.create_tensor([2, 5, 32]), 4,
                    kv_heads=kw.get("kv_heads"), key_lengths=L)
        m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])


@functools.lru_cache(maxsize=None)
def train(dev, graph=False, world=1, B=16, T=48, E=64, heads=2, steps=3):
    """3 SGD steps of two blocks of causal MQA self-attention (lengths changing every step, 0 and T among
    them) + ReLU dense in fp32; with world > 1 every op split on the samples.  Weights and the last loss."""
    from flexmi.core import ActiMode, LossType, SGDOptimizer
    from flexmi.core.types import DataType
    from flexmi.parallel.layout import ParallelConfig
    m = _model(B, dev)
    x = h = m.create_tensor([B, T, E])
    L = m.create_tensor([B, 1], DataType.DT_INT32)
    for i in range(2):
        h = m.dense(m.multihead_attention(h, h, h, E, heads, bias=False, causal=True, name=f"mha{i}", num_kv_heads=1,
                                          key_lengths=L), E, ActiMode.AC_MODE_RELU)
    m.dense(h, 1)
    m.compile(SGDOptimizer(m, 0.002), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    m.strategies = {op.name: ParallelConfig.data_parallel(op.out_ndims, world) for op in m.layers}
    ex = m.init_layers()
    attn = m.layers[3]
    assert tuple(ex.need[(attn.guid, 3)].degrees) == (world, 1) and tuple(ex.need[(attn.guid, 1)].shape) == (B, T, E // heads)
    rng = np.random.RandomState(0)
    run = ex.train_step
    for step in range(steps):
        ex.scatter_from_host(x, rng.randn(B, T, E).astype(np.float32))
        ex.scatter_from_host(L, np.r_[0, T, rng.randint(1, T, B - 2)].astype(np.int32).reshape(B, 1))
        ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, T, 1).astype(np.float32))
        run()
        run = ex.capture_step() if graph and step == 0 else run
    if dev == "gpu":
        torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters], m.get_perf_metrics().get_loss()


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        params = train("cpu", world=world)[0]
        if rank == 0:
            np.savez(out, *params)
    finally:
        dist.destroy_process_group()


@pytest.mark.multiproc
def test_world2_equals_world1():
    out = tempfile.mktemp(suffix=".npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    d = np.load(out)
    os.unlink(out)
    for i, b in enumerate(train("cpu")[0]):
        np.testing.assert_allclose(d[f"arr_{i}"], b, rtol=1e-4, atol=1e-5)
