"""RowwiseAdagradOptimizer over gloo: world 2 under table-wise and row-split table placements and
under pure data parallelism must train like world 1; under data parallelism the two replicas'
tables and accumulators are bit-identical (the gathered segments are summed in rank order on both);
a column split is rejected; and a checkpoint written at world 2 with a row split resumes at
world 1.  Every table is sparse with an accumulator ``h`` of shape [rows held, 1]."""
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
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, RowwiseAdagradOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    from flexmi.parallel.layout import ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny"))
    strat = {}
    if world > 1 and placement != "dp":
        # every table whole on one rank (no table is big enough for the plan's column split)
        strat = dlrm_strategy(m, world, split_factor=1e9)
        assert all(pc.dims == [1, 1] for pc in strat.values())
        if placement == "colsplit":
            strat["embedding1"] = ParallelConfig([world, 1], list(range(world)))
        elif placement == "rowsplit":
            strat["embedding2"] = ParallelConfig([1, 1, world], list(range(world)))
    m.strategies = strat
    m.compile(RowwiseAdagradOptimizer(m, 0.05, initial_accumulator_value=0.1), LossType.LOSS_BINARY_CROSSENTROPY,
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
        if e.box is None:                  # this rank holds no shard of the table
            continue
        assert e.op.rule.kind == "rowwise" and e.op.rule.eps == 1e-10 and not e.op.rule.host
        assert e.sparse and e.grad is None and e.group is None and id(e) not in in_groups
        assert set(e.state) == {"h"} and tuple(e.state["h"].shape) == (e.shape[0], 1)
        if e.layout.replication() == 1:
            assert e.op.rule == TableRule("rowwise", 1e-10, None)
        else:
            assert e.op.rule == TableRule("rowwise", 1e-10, tuple(range(world)))
    return sum(e.layout.replication() > 1 for e in embs)


def _job(rank, world, placement, ckpt, mode, out):
    m, d, s = _model(world, placement)
    if placement == "colsplit":            # every rank rejects it, holder of a shard or not
        with pytest.raises(NotImplementedError, match="column-split"):
            m.init_layers()
        return
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
    if placement == "dp":                  # this replica's own copies, for the bit-identity check
        from flexmi.core.types import OperatorType
        embs = [e for e in m._ex().wentries.values() if e.op.op_type == OperatorType.OP_EMBEDDING]
        np.savez(out + f".r{rank}.npz", *([e.master.numpy() for e in embs] + [e.state["h"].numpy() for e in embs]))


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
    if placement == "colsplit":
        return None
    d = np.load(out)
    res = {k: d[k] for k in d.files}
    os.unlink(out)
    if placement == "dp":
        res["replicas"] = []
        for r in range(world):
            f = out + f".r{r}.npz"
            d = np.load(f)
            res["replicas"].append([d[k] for k in sorted(d.files, key=lambda k: int(k.split("_")[1]))])
            os.unlink(f)
    return res


@pytest.fixture(scope="module")
def world1():
    return _launch(1, "dp")


def _compare(got, ref):
    keys = sorted((k for k in ref if k.startswith("arr_")), key=lambda k: int(k.split("_")[1]))
    assert len(keys) == len([k for k in got if k.startswith("arr_")])
    for k in keys:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("placement", ["table", "rowsplit", "dp"])
def test_world2_equals_world1(world1, placement):
    got = _launch(2, placement)
    _compare(got, world1)
    assert abs(float(got["loss"]) - float(world1["loss"])) < 1e-4
    if placement == "dp":
        a, b = got["replicas"]
        assert len(a) == len(b) == 8       # 4 tables + 4 accumulators
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y), "replicas differ"
        assert any(float(h.max()) > np.float32(0.1) for h in a[4:])     # the accumulators moved


def test_column_split_is_rejected():
    _launch(2, "colsplit")                 # the workers assert the NotImplementedError


def test_checkpoint_world2_rowsplit_to_world1(world1, tmp_path):
    ck = str(tmp_path / "ck")
    _launch(2, "rowsplit", ck, "save")
    got = _launch(1, "dp", ck, "load")
    _compare(got, world1)
