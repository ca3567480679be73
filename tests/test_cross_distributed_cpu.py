"""The DLRM ``dcn`` interaction (DCNv2 cross layers, ``CrossCombine``) over gloo: ``tiny_dcn`` at
world 2 trains like world 1 under table-wise placement, under pure data parallelism and with every
CrossCombine and its ``U`` Linear split two ways on the feature dimension; and with the exchange
chunked (``XCHG_CHUNKS = 2``) the whole cross stack runs inside the micro-batch pipelined tail."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.multiproc


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(world, placement, B):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    from flexmi.parallel.layout import ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny_dcn"))
    strat = {}
    if world > 1 and placement != "dp":
        strat = dlrm_strategy(m, world, split_factor=1e9)    # every table whole on one rank
        assert all(pc.dims == [1, 1] for pc in strat.values())
        if placement == "feature":
            for op in m.layers:
                if op.op_type == OperatorType.OP_CROSS_COMBINE:
                    u = op.inputs[1].owner_op
                    assert u.op_type == OperatorType.OP_LINEAR and u.use_bias
                    strat[op.name] = ParallelConfig([world, 1], list(range(world)))
                    strat[u.name] = ParallelConfig([world, 1], list(range(world)))
    m.strategies = strat
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.strategies = strat
    return m, d, s


def _job(rank, world, placement, B, out):
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig
    from flexmi.runtime import executor as E
    piped = placement == "pipe"
    E.XCHG_CHUNKS = "2" if piped else os.environ.get("FLEXMI_XCHG_CHUNKS", "auto")
    m, d, s = _model(world, placement, B)
    ex = m.init_layers()
    for op in m.layers:                    # the strategy is really applied (no silent fall-back)
        if op.name in m.strategies:
            assert ex.pcs[op.guid] == m.strategies[op.name], (op.name, ex.pcs[op.guid])
    if piped and world > 1:
        assert ex.pipe is not None and ex.pipe["K"] == 2 and ex.pipe["kb"] is not None, ex.pipe
        combines = [op for op in m.layers if op.op_type == OperatorType.OP_CROSS_COMBINE]
        assert len(combines) == 2 and all(op in ex.pipe["region"] for op in combines), ex.pipe["region"]
        names = [it.name for it in ex.prog_fwd + ex.prog_bwd]
        for c in range(2):
            for op in combines:
                assert f"{op.name}.c{c}.fwd" in names and f"{op.name}.c{c}.bwd" in names, names
    rows = DLRMConfig.preset("tiny_dcn").embedding_size
    for it in range(3):
        rng = np.random.RandomState(100 + it)
        ex.scatter_from_host(d, rng.rand(B, d.dims[1]).astype(np.float32))
        for t, r in zip(s, rows):
            ex.scatter_from_host(t, rng.randint(0, r, (B, 1)).astype(np.int64))
        ex.scatter_from_host(m.get_label_tensor(), rng.randint(0, 2, (B, 1)).astype(np.float32))
        ex.train_step()
    params = [p.get_weights(m) for p in m.parameters]
    loss = m.get_perf_metrics().get_loss()
    if rank == 0:
        np.savez(out, loss=loss, *params)


def _worker(rank, world, port, *args):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rc = 0
    try:
        _job(rank, world, *args)
    except BaseException:  # noqa: BLE001 -- reported through the exit code
        import traceback
        traceback.print_exc()
        rc = 1
    finally:
        dist.destroy_process_group()   # ordered teardown: normal interpreter exit afterwards
    sys.exit(rc)


def _launch(world, placement, B):
    out = tempfile.mktemp(suffix=".npz")
    if world == 1:
        _job(0, 1, placement, B, out)
    else:
        mp.start_processes(_worker, args=(world, _port(), placement, B, out), nprocs=world, join=True,
                           start_method="spawn")
    d = np.load(out)
    res = {k: d[k] for k in d.files}
    os.unlink(out)
    return res


@pytest.fixture(scope="module")
def world1():
    return {B: _launch(1, "dp", B) for B in (16, 128)}


def _compare(got, ref):
    keys = sorted((k for k in ref if k.startswith("arr_")), key=lambda k: int(k.split("_")[1]))
    assert len(keys) == len([k for k in got if k.startswith("arr_")]) == 18
    for k in keys:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)
    assert abs(float(got["loss"]) - float(ref["loss"])) < 1e-4


@pytest.mark.parametrize("placement", ["table", "dp", "feature"])
def test_world2_equals_world1(world1, placement):
    _compare(_launch(2, placement, 16), world1[16])


def test_cross_stack_runs_in_the_pipelined_tail(world1):
    _compare(_launch(2, "pipe", 128), world1[128])
