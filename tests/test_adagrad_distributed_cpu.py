"""AdagradOptimizer over gloo: world 2 under table-wise, column-split and row-split table
placements and under pure data parallelism must train like world 1, and a checkpoint written at
world 2 resumes at world 1.  Non-replicated tables are updated sparsely with their accumulator
``h``; replicated tables stay in a dense group (the replica all-reduce sums the gradients before
they are squared)."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.multiproc

B = 16


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(world, placement):
    from flexmi.core import AdagradOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    from flexmi.parallel.layout import ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny"))
    strat = {}
    if world > 1 and placement != "dp":
        strat = dlrm_strategy(m, world)
        if placement == "colsplit":
            strat["embedding1"] = ParallelConfig([world, 1], list(range(world)))
        elif placement == "rowsplit":
            strat["embedding2"] = ParallelConfig([1, 1, world], list(range(world)))
    m.strategies = strat
    m.compile(AdagradOptimizer(m, 0.05, initial_accumulator_value=0.1), LossType.LOSS_BINARY_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY])
    m.strategies = strat
    return m, d, s


def _steps(m, d, s, first, n):
    from flexmi.models.dlrm import DLRMConfig
    rows = DLRMConfig.preset("tiny").embedding_size
    ex = m._ex()
    for it in range(first, first + n):
        rng = np.random.RandomState(100 + it)
        dd = np.zeros((B, d.dims[1]), np.float32)
        dd[:, :13] = rng.rand(B, 13)
        ex.scatter_from_host(d, dd)
        for t, r in zip(s, rows):
            ex.scatter_from_host(t, rng.randint(0, r, (B, 1)).astype(np.int64))
        ex.scatter_from_host(m.get_label_tensor(), rng.randint(0, 2, (B, 1)).astype(np.float32))
        ex.train_step()


def _check_entries(m, world):
    from flexmi.core.types import OperatorType
    from flexmi.ops.embedding import TableRule
    ex = m._ex()
    embs = [e for e in ex.wentries.values() if e.op.op_type == OperatorType.OP_EMBEDDING]
    assert len(embs) == 4
    in_groups = {id(e) for g in ex.groups for e in g.entries}
    for e in embs:
        if e.layout.replication() == 1:
            if e.box is not None:          # this rank holds a shard of the table
                assert e.op.rule == TableRule("adagrad", 1e-10, None)
                assert e.sparse and e.grad is None and e.group is None and id(e) not in in_groups
                assert set(e.state) == {"h"} and tuple(e.state["h"].shape) == tuple(e.shape)
        else:
            assert not e.sparse and e.op.rule is None
            assert id(e) in in_groups and e.grad is not None
    return sum(e.layout.replication() > 1 for e in embs)


def _job(rank, world, placement, ckpt, mode, out):
    m, d, s = _model(world, placement)
    m.init_layers()
    replicated = _check_entries(m, world)
    assert replicated == (4 if world > 1 and placement == "dp" else 0)
    if mode == "full":
        _steps(m, d, s, 0, 3)
    elif mode == "save":
        _steps(m, d, s, 0, 2)
        m.save_checkpoint(ckpt)
    else:
        m.load_checkpoint(ckpt)
        _steps(m, d, s, 2, 1)
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


def _launch(world, placement, ckpt=None, mode="full"):
    out = tempfile.mktemp(suffix=".npz")
    if world == 1:
        _job(0, 1, placement, ckpt, mode, out)
    else:
        mp.start_processes(_worker, args=(world, _port(), placement, ckpt, mode, out), nprocs=world, join=True,
                           start_method="spawn")
    d = np.load(out)
    res = {k: d[k] for k in d.files}
    os.unlink(out)
    return res


@pytest.fixture(scope="module")
def world1():
    return _launch(1, "dp")


def _compare(got, ref):
    keys = sorted((k for k in ref if k.startswith("arr_")), key=lambda k: int(k.split("_")[1]))
    assert len(keys) == len([k for k in got if k.startswith("arr_")])
    for k in keys:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("placement", ["table", "colsplit", "rowsplit", "dp"])
def test_world2_equals_world1(world1, placement):
    got = _launch(2, placement)
    _compare(got, world1)
    assert abs(float(got["loss"]) - float(world1["loss"])) < 1e-4


def test_checkpoint_world2_table_to_world1(world1, tmp_path):
    ck = str(tmp_path / "ck")
    _launch(2, "table", ck, "save")
    got = _launch(1, "dp", ck, "load")
    _compare(got, world1)
