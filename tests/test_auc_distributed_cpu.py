"""METRICS_AUC over gloo: at world 2 and 4, under data parallelism and under ``dlrm_strategy``, the
int64 histogram folded by one all-reduce equals the oracle binning of the predictions gathered in
that same run, on every rank, and every rank reports bit-identical AUC and bound.  (No comparison
against a world-1 run: a last-bit difference in a prediction may move a sample across a bin edge;
the integer comparison inside one run is the stronger check.)"""
import os
import socket
import struct
import sys
import tempfile

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.multiproc

B = 16
EVAL_STEPS, TRAIN_STEPS = 3, 2


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(world, placement):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny"))
    strat = dlrm_strategy(m, world) if placement == "strategy" else {}
    m.strategies = strat
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_BINARY_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC])
    m.strategies = strat
    return m, d, s


def _feed(m, d, s, it):
    from flexmi.models.dlrm import DLRMConfig
    ex = m._ex()
    rng = np.random.RandomState(100 + it)
    dd = np.zeros((B, d.dims[1]), np.float32)
    dd[:, :13] = rng.rand(B, 13)
    ex.scatter_from_host(d, dd)
    for t, r in zip(s, DLRMConfig.preset("tiny").embedding_size):
        ex.scatter_from_host(t, rng.randint(0, r, (B, 1)).astype(np.int64))
    lab = (rng.rand(B, 1) < 0.4).astype(np.float32)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    return lab


def _job(rank, world, placement, out):
    import torch
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT, auc_from_hist, auc_hist_torch
    m, d, s = _model(world, placement)
    ex = m.init_layers()
    m.reset_metrics()
    preds, labs = [], []
    ex.training = False
    for it in range(EVAL_STEPS):
        labs.append(_feed(m, d, s, it))
        m.forward()
        m.compute_metrics()
        preds.append(ex.gather_to_host(m.get_output_tensor()).copy())
    ex.training = True
    for it in range(EVAL_STEPS, EVAL_STEPS + TRAIN_STEPS):
        labs.append(_feed(m, d, s, it))
        m.forward()
        preds.append(ex.gather_to_host(m.get_output_tensor()).copy())   # this step's predictions, before the update
        m.zero_gradients()
        m.backward()
        m.update()
    p, y = torch.from_numpy(np.concatenate(preds)), torch.from_numpy(np.concatenate(labs))
    want = torch.zeros(2, AUC_BINS, dtype=torch.int64)
    winv = torch.zeros(1, dtype=torch.int64)
    auc_hist_torch(p, y, want, winv, AUC_SHIFT)
    hist, inv = ex.auc_hist_folded()
    total = B * (EVAL_STEPS + TRAIN_STEPS)
    assert torch.equal(hist, want), f"rank {rank}: folded histogram differs from the oracle"
    assert int(inv) == 0 and int(ex.auc_hist.sum()) <= total          # the local state is this rank's part
    pm = m.get_perf_metrics()
    assert pm.auc_pos + pm.auc_neg == total and pm.auc_pos == int(y.sum())
    assert (pm.get_auc(), pm.get_auc_bound()) == auc_from_hist(want)[:2]
    with open(f"{out}.{rank}", "wb") as f:
        f.write(struct.pack("<dd", pm.get_auc(), pm.get_auc_bound()))


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


@pytest.mark.parametrize("placement", ["dp", "strategy"])
@pytest.mark.parametrize("world", [2, 4])
def test_folded_histogram_is_exact_and_identical_on_every_rank(world, placement):
    out = tempfile.mktemp(suffix=".auc")
    mp.start_processes(_worker, args=(world, _port(), placement, out), nprocs=world, join=True, start_method="spawn")
    got = []
    for r in range(world):
        with open(f"{out}.{r}", "rb") as f:
            got.append(f.read())
        os.unlink(f"{out}.{r}")
    assert len(set(got)) == 1, [struct.unpack("<dd", g) for g in got]      # bit-identical on every rank
    auc, bound = struct.unpack("<dd", got[0])
    assert 0.0 <= auc <= 1.0 and 0.0 <= bound <= 1.0
