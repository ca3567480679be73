"""Per-table multi-hot bag sizes over gloo: ``tiny_dcn_multihot`` (bags 3, 1, 8, 2) at world 2 trains
like world 1 under table-wise placement and under pure data parallelism, with SGD and -- for the
data-parallel case, where the replicated tables go through the rank-ordered merge of touched rows --
with row-wise Adagrad."""
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


def _model(world, placement, optname):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, RowwiseAdagradOptimizer, SGDOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny_dcn_multihot"))
    strat = {}
    if world > 1 and placement == "table":
        strat = dlrm_strategy(m, world, split_factor=1e9)    # every table whole on one rank
        assert len(strat) == 4 and all(pc.dims == [1, 1] for pc in strat.values())
    m.strategies = strat
    opt = SGDOptimizer(m, 0.1) if optname == "sgd" else RowwiseAdagradOptimizer(m, 0.1)
    m.compile(opt, LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.strategies = strat
    return m, d, s


def _job(rank, world, placement, optname, out):
    from flexmi.models.dlrm import DLRMConfig
    m, d, s = _model(world, placement, optname)
    ex = m.init_layers()
    for op in m.layers:                    # the strategy is really applied (no silent fall-back)
        if op.name in m.strategies:
            assert ex.pcs[op.guid] == m.strategies[op.name], (op.name, ex.pcs[op.guid])
    dcfg = DLRMConfig.preset("tiny_dcn_multihot")
    assert [tuple(t.dims) for t in s] == [(B, b) for b in (3, 1, 8, 2)]
    for it in range(3):
        rng = np.random.RandomState(100 + it)
        ex.scatter_from_host(d, rng.rand(B, d.dims[1]).astype(np.float32))
        for t, r, bag in zip(s, dcfg.embedding_size, dcfg.bag_sizes()):
            a = rng.randint(0, r, (B, bag)).astype(np.int64)
            if bag > 1:
                a[it, -1] = a[it, 0]       # one bag holds the same row twice
                a[B - 1] = a[0]            # and two samples (one per rank under DP) share their rows
            ex.scatter_from_host(t, a)
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


def _launch(world, placement, optname):
    out = tempfile.mktemp(suffix=".npz")
    if world == 1:
        _job(0, 1, placement, optname, out)
    else:
        mp.start_processes(_worker, args=(world, _port(), placement, optname, out), nprocs=world, join=True,
                           start_method="spawn")
    d = np.load(out)
    res = {k: d[k] for k in d.files}
    os.unlink(out)
    return res


@pytest.fixture(scope="module")
def world1():
    return {o: _launch(1, "dp", o) for o in ("sgd", "rowwise_adagrad")}


def _compare(got, ref):
    keys = sorted((k for k in ref if k.startswith("arr_")), key=lambda k: int(k.split("_")[1]))
    assert len(keys) == len([k for k in got if k.startswith("arr_")]) == 18
    for k in keys:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)
    assert abs(float(got["loss"]) - float(ref["loss"])) < 1e-4


@pytest.mark.parametrize("placement,optname", [("table", "sgd"), ("dp", "sgd"), ("dp", "rowwise_adagrad")])
def test_world2_equals_world1(world1, placement, optname):
    _compare(_launch(2, placement, optname), world1[optname])
