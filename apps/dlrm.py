#!/usr/bin/env python3
"""The reference DLRM application (``examples/cpp/DLRM/dlrm.cc:77-199``) on flexmi.

    python apps/dlrm.py --arch-sparse-feature-size 64 --arch-embedding-size 1000000-1000000 \\
        --arch-mlp-bot 64-512-512-64 --arch-mlp-top 576-1024-1024-1024-1 -b 2048 -e 1 [--dataset f.h5]
    python apps/dlrm.py --preset summit_large -b 256 -e 1
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 apps/dlrm.py --preset run_random -b 2048 --strategy s.pb

Same flags as the reference (``parse_input_args`` dlrm.cc:201-264 + the FFConfig flag set):
``--dataset`` trains on the HDF5 file written by ``preprocess_hdf.py`` (native reader + prefetch
ring, ``HDF5DLRMData``), otherwise on random data of ``--data-size`` samples (default 256 x 4 x
GPUs, dlrm.cc:273-282); ``--loss-threshold t`` clamps predictions to [t, 1-t] in the loss.  The
loop is the reference's (dlrm.cc:160-195): per epoch ``num_samples / batch`` iterations of
next_batch / forward / zero_gradients / backward / update, traced with begin/end_trace(111),
then ``ELAPSED TIME = ..., THROUGHPUT = ... samples/s``.  ``--preset`` (mlperf, mlperf_dcnv2,
mlperf_dcnv2_multihot, run_random, criteo_kaggle, summit, summit_large, kaggle_day1, tiny, tiny_dcn,
tiny_dcn_multihot) seeds the architecture flags.
``--embedding-bag-sizes 3-2-1-...`` (flexmi extension) gives every table its own bag size (the fixed
multi-hot sizes of the MLPerf DCNv2 data set; the ``*_multihot`` presets set them); a later
``--embedding-bag-size N`` goes back to one size for all.  X_cat of ``--dataset`` is then [N, sum of the sizes].
``--arch-interaction-op dcn`` (flexmi extension, with ``--arch-dcn-layers N`` and ``--arch-dcn-rank R``) puts N
DCNv2 low-rank cross layers between the concatenation and the top MLP (MLPerf DLRM-DCNv2).
``--optimizer {sgd,adagrad,rowwise_adagrad}`` (flexmi extension, default sgd): Adagrad keeps one
accumulator per table element and updates non-replicated tables sparsely; row-wise Adagrad keeps
one per table ROW and trains every table sparsely, replicated ones included
(``flexmi/core/optimizers.py``).
``--auc`` (flexmi extension) adds the streaming ROC AUC to the training metrics and to the final
stderr line.  ``--eval-dataset FILE.h5`` (implies ``--auc``) runs a held-out pass over the file's
whole batches after every epoch (``--eval-data-size N`` caps it) and prints ``EVAL epoch E: loss ...
accuracy ... auc ... (+-bound)``; ``--auc-threshold A`` stops after the first epoch whose
evaluation AUC is >= A (the MLPerf stopping rule).  ``main()`` returns ``(samples/s, metrics)``;
``metrics.eval`` is the last evaluation's ``PerfMetrics`` (None without ``--eval-dataset``).
"""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    import torch
    from flexmi.core import (AdagradOptimizer, FFConfig, FFModel, LossType, MetricsType, RowwiseAdagradOptimizer,
                             SGDOptimizer)
    from flexmi.models.dlrm import DLRMConfig, HDF5DLRMData, SyntheticDLRMData, build_dlrm
    from flexmi.parallel.comm import init_distributed

    comm = init_distributed()
    base = None
    if "--preset" in argv:
        k = argv.index("--preset")
        base = DLRMConfig.preset(argv[k + 1])
        del argv[k:k + 2]
    optname = "sgd"
    if "--optimizer" in argv:
        k = argv.index("--optimizer")
        optname = argv[k + 1]
        del argv[k:k + 2]
        if optname not in ("sgd", "adagrad", "rowwise_adagrad"):
            raise SystemExit(f"--optimizer {optname}: expected sgd, adagrad or rowwise_adagrad")
    want_auc = "--auc" in argv
    if want_auc:
        argv.remove("--auc")
    eval_path, eval_size, auc_threshold = None, 0, None
    for flag in ("--eval-dataset", "--eval-data-size", "--auc-threshold"):
        if flag in argv:
            k = argv.index(flag)
            v = argv[k + 1]
            del argv[k:k + 2]
            if flag == "--eval-dataset":
                eval_path = v
            elif flag == "--eval-data-size":
                eval_size = int(v)
            else:
                auc_threshold = float(v)
    if auc_threshold is not None and not eval_path:
        raise SystemExit("--auc-threshold needs --eval-dataset: the threshold is on the evaluation AUC")
    want_auc = want_auc or bool(eval_path)
    dcfg = DLRMConfig.parse_args(["dlrm"] + argv, base)
    cfg = FFConfig()
    cfg.parse_args(["dlrm"] + argv)
    if dcfg.dataset_path and not cfg.dataset_path:
        cfg.dataset_path = dcfg.dataset_path
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    model = FFModel(cfg)
    dense_in, sparse, out = build_dlrm(model, dcfg)
    loss = LossType.LOSS_BINARY_CROSSENTROPY if dcfg.loss == "bce" else LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE
    opt = {"sgd": SGDOptimizer, "adagrad": AdagradOptimizer,
           "rowwise_adagrad": RowwiseAdagradOptimizer}[optname](model, cfg.learningRate)
    model.compile(opt, loss,
                  [MetricsType.METRICS_ACCURACY, MetricsType.METRICS_MEAN_SQUARED_ERROR] +
                  ([MetricsType.METRICS_AUC] if want_auc else []))
    ex = model.init_layers()
    edata = None
    if eval_path:
        import copy
        ecfg = copy.copy(dcfg)
        ecfg.data_size = eval_size
        edata = HDF5DLRMData(model, dense_in, sparse, ecfg, path=eval_path)

    def evaluate(epoch):
        """Held-out pass over the whole batches of --eval-dataset: forward + metrics only."""
        ex.training = False
        model.reset_metrics()
        edata.loader.reset()
        for _ in range(edata.nb):
            edata.next_batch()
            model.forward()
            model.compute_metrics()
        em = model.get_perf_metrics()
        if comm.rank == 0:
            print(f"EVAL epoch {epoch}: loss {em.get_loss():.5f} accuracy {em.get_accuracy():.2f}% "
                  f"auc {em.get_auc():.5f} (+-{em.get_auc_bound():.1e})", flush=True)
        ex.training = True
        model.reset_metrics()
        return em

    if dcfg.dataset_path:
        data = HDF5DLRMData(model, dense_in, sparse, dcfg)
        num_samples = data.num_samples
    else:
        num_samples = dcfg.data_size if dcfg.data_size > 0 else 256 * 4 * cfg.workersPerNode * cfg.numNodes
        num_samples = max(num_samples, cfg.batchSize)
        data = SyntheticDLRMData(model, dense_in, sparse, dcfg, num_batches=max(1, num_samples // cfg.batchSize),
                                 seed=comm.rank)
    iters = max(1, num_samples // cfg.batchSize)
    sync = torch.cuda.synchronize if ex.backend == "hip" else (lambda: None)
    # warm-up iteration (dlrm.cc:153-158), not timed
    data.next_batch()
    ex.train_step()
    sync()
    comm.barrier()
    t0 = time.perf_counter()
    m = em = None
    t_eval = 0.0
    epochs_done = 0
    for epoch in range(cfg.epochs):
        model.reset_metrics()
        for it in range(iters):
            if epoch > 0 or it > 0:
                model.begin_trace(111)
            data.next_batch()
            model.forward()
            model.zero_gradients()
            model.backward()
            model.update()
            if epoch > 0 or it > 0:
                model.end_trace(111)
        epochs_done = epoch + 1
        if edata is not None:
            # the evaluation pass resets the metrics: keep this epoch's training metrics, and keep
            # the pass out of the training time
            sync()
            te = time.perf_counter()
            m = model.get_perf_metrics()
            em = evaluate(epoch)
            sync()
            t_eval += time.perf_counter() - te
            if auc_threshold is not None and em.get_auc() >= auc_threshold:
                break               # MLPerf stopping rule: first epoch that reaches the target
    sync()
    comm.barrier()
    el = time.perf_counter() - t0 - t_eval
    if m is None:
        m = model.get_perf_metrics()
    m.eval = em                     # last evaluation PerfMetrics, None without --eval-dataset
    samples = num_samples * epochs_done
    if comm.rank == 0:
        auc_s = f" auc {m.get_auc():.5f} (+-{m.get_auc_bound():.1e})" if want_auc else ""
        print(f"[dlrm {dcfg.name}] {epochs_done} epoch(s) x {iters} iterations, batch {cfg.batchSize}, "
              f"{comm.world} device(s), {'dataset ' + dcfg.dataset_path if dcfg.dataset_path else 'random data'}: "
              f"loss {m.get_loss():.5f} accuracy {m.get_accuracy():.2f}%{auc_s}", file=sys.stderr)
        print(f"ELAPSED TIME = {el:.4f}s, THROUGHPUT = {samples / el:.2f} samples/s", flush=True)
    if hasattr(data, "close"):
        data.close()
    if edata is not None:
        edata.close()
    return samples / el, m


if __name__ == "__main__":
    main()
