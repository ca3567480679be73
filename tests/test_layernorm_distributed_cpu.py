"""LayerNorm over gloo: a post-norm encoder layer trained data-parallel at world 2 ends where world 1 does."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.multiproc
B, T, E, HEADS, FF = 8, 6, 16, 2, 24


def _job(rank, world, out):
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    from flexmi.core.types import OperatorType
    from flexmi.parallel.layout import Layout, ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, 5
    m = FFModel(cfg)
    x = m.create_tensor([B, T, E])
    m.dense(m.transformer_encoder_layer(x, HEADS, FF, causal=True, name="enc"), 1)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    m.strategies = {op.name: ParallelConfig.data_parallel(op.out_ndims, world) for op in m.layers}
    ex = m.init_layers()
    norms = [op for op in m.layers if op.op_type == OperatorType.OP_LAYERNORM]
    assert len(norms) == 2 and all(tuple(Layout.from_pc(op.outputs[0].dims, ex.pcs[op.guid]).degrees) == (world, 1, 1)
                                   for op in norms)                             # really split on the samples
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


def test_world2_equals_world1():
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
    assert len(res[0]) == len(res[1]) == 18
    for a, b in zip(res[1], res[0]):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
