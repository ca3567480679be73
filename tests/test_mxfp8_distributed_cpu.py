"""LinearMX over gloo: data parallel at world 2 (64 rows per rank) gives the single-process forward bit for bit
(a block's scale depends on its own 32 values only) and the same weights after one step."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.multiproc
B, D, H = 128, 64, 96


def _job(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    from flexmi.core.types import ActiMode, OperatorType
    from flexmi.parallel.layout import ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize, cfg.seed = "cpu", "fp32", B, 5
    m = FFModel(cfg)
    x = m.create_tensor([B, D])
    y = m.dense(m.dense(x, H, ActiMode.AC_MODE_RELU, fp8=True), 32, fp8=True)
    assert all(op.op_type == OperatorType.OP_LINEAR_MX for op in m.layers)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    m.strategies = {op.name: ParallelConfig.data_parallel(op.out_ndims, world) for op in m.layers}
    ex = m.init_layers()
    rng = np.random.RandomState(3)
    ex.scatter_from_host(x, rng.randn(B, D).astype(np.float32))
    ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, 32).astype(np.float32))
    ex.train_step()
    res = [ex.gather_to_host(y)] + [p.get_weights(m) for p in m.parameters]
    if rank == 0:
        np.savez(out, *res)
    if world > 1:
        dist.destroy_process_group()


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
    assert len(res[0]) == len(res[1]) == 5 and np.array_equal(res[0][0], res[1][0]), "forward output"
    for a, b in zip(res[1][1:], res[0][1:]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5)
