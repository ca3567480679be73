"""Streaming ROC AUC (METRICS_AUC) on the CPU: the torch oracle against an exact rank-statistic AUC
in rational arithmetic, the key order, the native CPU kernel, the executor state, and the front
ends (Keras, MetricsLogger, C API, apps/dlrm.py)."""
import json
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64


def logistic_set(n, seed=0):
    """y ~ Bernoulli(0.25), z ~ N(0, 1.5) + y - 2, p = sigmoid(z) as fp32; both classes present."""
    rng = np.random.RandomState(seed)
    y = rng.rand(n) < 0.25
    y[0], y[1 % n] = True, False
    z = rng.normal(0.0, 1.5, n) + y - 2.0
    p = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    return torch.from_numpy(p), torch.from_numpy(y.astype(np.float32))


def exact_auc(scores, labels):
    """Rank-statistic AUC with ties counted 1/2, as a Fraction (None when a class is missing)."""
    groups = {}
    for s, y in zip(scores.float().reshape(-1).tolist(), labels.float().reshape(-1).tolist()):
        groups.setdefault(s, [0, 0])[1 if y >= 0.5 else 0] += 1      # -0.0 == 0.0: one group
    below, num, P, N = 0, 0, 0, 0
    for s in sorted(groups):
        n, p = groups[s]
        num += p * (2 * below + n)
        below += n
        P += p
        N += n
    return Fraction(num, 2 * P * N) if P and N else None


def _state(shift=None):
    from flexmi.core.loss_metrics import AUC_SHIFT
    shift = AUC_SHIFT if shift is None else shift
    return torch.zeros(2, 1 << (32 - shift), dtype=torch.int64), torch.zeros(1, dtype=torch.int64)


# ------------------------------------------------------------------ 1. oracle against exact AUC
@pytest.mark.parametrize("n", [2, 63, 4096])
def test_oracle_within_bound_of_exact_auc(n):
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT, auc_from_hist, auc_hist_torch
    assert AUC_SHIFT == 12 and AUC_BINS == 1 << 20
    p, y = logistic_set(n)
    hist, inv = _state()
    auc_hist_torch(p, y, hist, inv, AUC_SHIFT)
    auc, bound, P, N = auc_from_hist(hist)
    assert P + N == n and P == int(y.sum()) and int(inv) == 0
    exact = exact_auc(p, y)
    print(f"n={n} auc={auc!r} exact={float(exact)!r} err={float(abs(Fraction(auc) - exact)):.3e} bound={bound:.3e}")
    assert abs(Fraction(auc) - exact) <= Fraction(bound) + Fraction(1e-12)
    if n == 4096:
        assert bound <= 1e-3
    # bf16 scores: 16 significant bits >= AUC_SHIFT, every distinct value has its own bin
    pb = p.bfloat16()
    hist, inv = _state()
    auc_hist_torch(pb, y, hist, inv, AUC_SHIFT)
    auc, bound, P, N = auc_from_hist(hist)
    assert abs(Fraction(auc) - exact_auc(pb, y)) <= Fraction(1e-12)


# ------------------------------------------------------------------ 2. key order
SPECIAL = [-math.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, math.inf]


def test_key_order_and_special_values():
    from flexmi.core.loss_metrics import AUC_SHIFT, auc_from_hist, auc_hist_torch, auc_keys
    s = torch.tensor(SPECIAL, dtype=torch.float32)
    bins = (auc_keys(s) >> AUC_SHIFT).tolist()
    assert bins == sorted(bins) and bins[3] == bins[4]
    assert bins[0] < bins[1] < bins[2] < bins[3] and bins[4] < bins[5] < bins[6] < bins[7]
    assert 0 <= bins[0] and bins[-1] < 1 << (32 - AUC_SHIFT)
    y = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1], dtype=torch.float32)
    hist, inv = _state()
    auc_hist_torch(s, y, hist, inv, AUC_SHIFT)
    assert int(hist.sum()) == 8 and int(inv) == 0
    for b, lab in zip(bins, y.tolist()):
        assert int(hist[int(lab), b]) >= 1
    auc, bound, P, N = auc_from_hist(hist)
    assert abs(Fraction(auc) - exact_auc(s, y)) <= Fraction(bound) + Fraction(1e-12)
    # NaN: counted as invalid and nowhere else
    before = hist.clone()
    auc_hist_torch(torch.tensor([math.nan, -math.nan]), torch.tensor([1.0, 0.0]), hist, inv, AUC_SHIFT)
    assert int(inv) == 2 and torch.equal(hist, before)
    # soft labels: >= 0.5 is positive (the rule of binary accuracy)
    hist, inv = _state()
    auc_hist_torch(torch.tensor([0.25, 0.75]), torch.tensor([0.3, 0.7]), hist, inv, AUC_SHIFT)
    assert hist.sum(1).tolist() == [1, 1] and auc_from_hist(hist)[:2] == (1.0, 0.0)
    assert int(hist[0, int(auc_keys(torch.tensor([0.25]))[0]) >> AUC_SHIFT]) == 1
    # a single class: NaN
    hist, inv = _state()
    auc_hist_torch(torch.tensor([0.1, 0.9]), torch.tensor([1.0, 1.0]), hist, inv, AUC_SHIFT)
    auc, bound, P, N = auc_from_hist(hist)
    assert math.isnan(auc) and math.isnan(bound) and (P, N) == (2, 0)


# ------------------------------------------------------------------ 3. native CPU kernel
@pytest.mark.parametrize("n", [1, 1000, 100000])
def test_native_cpu_kernel_equals_oracle(n):
    cpu = pytest.importorskip("flexmi._cpu")
    from flexmi.core.loss_metrics import AUC_SHIFT, auc_hist_torch
    p, y = logistic_set(n, seed=3)
    sp = torch.tensor(SPECIAL + [math.nan], dtype=torch.float32)
    q = torch.cat([p[: n // 2], sp.repeat(n // 18 + 1)[: n - n // 2]])          # second call: special values too
    want, winv = _state()
    got, ginv = _state()
    for s in (p, q):
        auc_hist_torch(s, y, want, winv, AUC_SHIFT)
        cpu.auc_hist(s.reshape(-1, 1), y.reshape(-1, 1), got, ginv, AUC_SHIFT)
    assert torch.equal(got, want) and int(ginv) == int(winv)
    assert int(got.sum()) + int(ginv) == 2 * n


# ------------------------------------------------------------------ 4-6. model level
def _tiny(metrics, batch=B, optimizer=None):
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", batch
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny"))
    m.compile(optimizer(m) if optimizer else SGDOptimizer(m, 0.05), LossType.LOSS_BINARY_CROSSENTROPY, metrics)
    return m, d, s


def _feed(m, d, s, it, batch=B):
    from flexmi.models.dlrm import DLRMConfig
    ex = m._ex()
    rng = np.random.RandomState(100 + it)
    dd = np.zeros((batch, d.dims[1]), np.float32)
    dd[:, :13] = rng.rand(batch, 13)
    ex.scatter_from_host(d, dd)
    for t, r in zip(s, DLRMConfig.preset("tiny").embedding_size):
        ex.scatter_from_host(t, rng.randint(0, r, (batch, 1)).astype(np.int64))
    lab = (rng.rand(batch, 1) < 0.3).astype(np.float32)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    return lab


def test_model_histogram_equals_oracle_of_gathered_predictions():
    from flexmi.core import MetricsType
    from flexmi.core.loss_metrics import AUC_SHIFT, auc_hist_torch
    m, d, s = _tiny([MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC])
    ex = m.init_layers()
    ex.training = False
    m.reset_metrics()
    preds, labs = [], []
    for it in range(5):
        labs.append(_feed(m, d, s, it))
        m.forward()
        m.compute_metrics()
        preds.append(ex.gather_to_host(m.get_output_tensor()).copy())
    p, y = torch.from_numpy(np.concatenate(preds)), torch.from_numpy(np.concatenate(labs))
    want, winv = _state()
    auc_hist_torch(p, y, want, winv, AUC_SHIFT)
    assert torch.equal(ex.auc_hist, want) and int(ex.auc_invalid) == 0
    pm = m.get_perf_metrics()
    assert pm.auc_pos + pm.auc_neg == 5 * B == pm.train_all and pm.auc_pos == int(y.sum()) and pm.auc_invalid == 0
    assert abs(Fraction(pm.get_auc()) - exact_auc(p, y)) <= Fraction(pm.get_auc_bound()) + Fraction(1e-12)
    assert f" auc: {pm.get_auc():.5f} (+-{pm.get_auc_bound():.1e})" in str(pm)
    m.reset_metrics()
    assert int(ex.auc_hist.sum()) == 0 and int(ex.auc_invalid) == 0
    pm = m.get_perf_metrics()
    assert math.isnan(pm.get_auc()) and pm.auc_pos + pm.auc_neg == 0
    # training steps accumulate too
    ex.training = True
    for it in range(3):
        _feed(m, d, s, 10 + it)
        ex.train_step()
    pm = m.get_perf_metrics()
    assert pm.auc_pos + pm.auc_neg == 3 * B and int(ex.auc_hist.sum()) == 3 * B


def test_no_footprint_when_not_requested():
    from flexmi.core import MetricsType
    from flexmi.core.loss_metrics import PerfMetrics
    m0, d0, s0 = _tiny([MetricsType.METRICS_ACCURACY])
    m1, _, _ = _tiny([MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC])
    e0, e1 = m0.init_layers(), m1.init_layers()
    assert e0.auc_hist is None and e0.auc_invalid is None and e0.auc_state is None
    assert e1.auc_hist is not None and tuple(e1.auc_hist.shape) == (2, 1 << 20) and e1.auc_hist.dtype == torch.int64
    def names(ex, prog):        # default op names end in a process-wide counter: "Dense_32_109.fwd"
        return [re.sub(r"_\d+(?=\.|$)", "", it.name) for it in getattr(ex, prog)]
    for prog in ("prog_fwd", "prog_bwd", "prog_upd"):
        assert names(e0, prog) == names(e1, prog) and "loss" in names(e0, "prog_fwd") + names(e0, "prog_bwd"), prog
    assert m0.metrics_op.mask == m1.metrics_op.mask and not m0.metrics_op.auc and m1.metrics_op.auc
    _feed(m0, d0, s0, 0)
    e0.train_step()
    pm = m0.get_perf_metrics()
    assert not pm.has_auc and "auc" not in str(pm) and math.isnan(pm.get_auc())
    assert not PerfMetrics(np.zeros(8), []).has_auc              # the two-argument form keeps working


def test_compile_rejects_auc_for_a_softmax_classifier():
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexmi.core.types import ActiMode, DataType
    for loss, width in ((LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, 4), (LossType.LOSS_CATEGORICAL_CROSSENTROPY, 4),
                        (LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, 1)):
        cfg = FFConfig()
        cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", 8
        m = FFModel(cfg)
        x = m.create_tensor([8, 6], DataType.DT_FLOAT)
        t = m.dense(x, width, ActiMode.AC_MODE_NONE)
        t = m.softmax(t)
        with pytest.raises(ValueError, match="METRICS_AUC"):
            m.compile(SGDOptimizer(m, 0.1), loss, [MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC])


# ------------------------------------------------------------------ 7. Keras
def test_keras_history_has_auc_only_when_requested():
    from flexmi.core import FFConfig
    from flexmi.core.types import MetricsType
    from flexmi.keras import Sequential, optimizers
    from flexmi.keras.layers import Dense
    from flexmi.keras.metrics import AUC, get
    assert isinstance(get("auc"), AUC) and AUC.type == MetricsType.METRICS_AUC == 1064
    rng = np.random.RandomState(0)
    x = rng.rand(128, 8).astype(np.float32)
    y = (x[:, :1] + 0.2 * rng.rand(128, 1) > 0.6).astype(np.float32)
    hists = {}
    for names in (["accuracy", "auc"], ["accuracy"]):
        cfg = FFConfig()
        cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", 32
        model = Sequential([Dense(16, input_shape=(8,), activation="relu"), Dense(1, activation="sigmoid")], ffconfig=cfg)
        model.compile(optimizer=optimizers.SGD(learning_rate=0.5), loss="binary_crossentropy", metrics=names)
        hists[len(names)] = (model.fit(x, y, epochs=2, verbose=0), model.evaluate(x, y, verbose=0))
    fit, ev = hists[2]
    assert len(fit) == 2 and all("auc" in h and 0.0 <= h["auc"] <= 1.0 for h in fit)
    assert "auc" in ev[0] and 0.0 <= ev[0]["auc"] <= 1.0
    fit, ev = hists[1]
    assert all("auc" not in h for h in fit) and "auc" not in ev[0]


# ------------------------------------------------------------------ 8. MetricsLogger
def test_metrics_logger_records_auc(tmp_path):
    from flexmi.core import MetricsType
    from flexmi.utils.log import MetricsLogger
    recs = {}
    for name, metrics in (("with", [MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC]),
                          ("without", [MetricsType.METRICS_ACCURACY])):
        m, d, s = _tiny(metrics)
        ex = m.init_layers()
        _feed(m, d, s, 0)
        ex.train_step()
        path = str(tmp_path / f"{name}.jsonl")
        log = MetricsLogger(path, rank=0)
        pm = m.get_perf_metrics()
        log.step(1, B, pm, ex)
        log.close()
        recs[name] = ([json.loads(ln) for ln in open(path) if '"step"' in ln][-1], pm)
    rec, pm = recs["with"]
    assert rec["auc"] == pm.get_auc() and rec["auc_bound"] == pm.get_auc_bound()
    assert "auc" not in recs["without"][0] and "auc_bound" not in recs["without"][0]


# ------------------------------------------------------------------ 9. C API
C_PROG = r"""
#include <stdio.h>
#include <stdlib.h>
#include "flexmi_c.h"
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s failed: %s\n", #x, flexmi_last_error()); return 1; } } while (0)
int main(int argc, char** argv) {
  CHECK(flexmi_init(argc, argv) == 0);
  flexmi_config_t cfg = flexmi_config_create();
  CHECK(cfg && flexmi_config_parse_args_default(cfg) == 0);
  const int B = flexmi_config_get_batch_size(cfg), F = 8, N = 256;
  flexmi_model_t m = flexmi_model_create(cfg);
  int dims[2] = {B, F};
  flexmi_tensor_t x = flexmi_tensor_create(m, 2, dims, 40, 1, "input");
  flexmi_tensor_t t = flexmi_model_add_dense(m, x, 16, 11, 1, NULL, NULL, "dense1");
  t = flexmi_model_add_dense(m, t, 1, 12, 1, NULL, NULL, "dense2");
  CHECK(t);
  flexmi_optimizer_t sgd = flexmi_sgd_optimizer_create(m, 0.5, 0.0, 0, 0.0);
  int metrics[2] = {1001, 1064};
  CHECK(flexmi_model_compile(m, sgd, 54, metrics, 2) == 0);
  CHECK(flexmi_model_init_layers(m) == 0);
  float* xs = (float*)malloc(sizeof(float) * N * F);
  float* ys = (float*)malloc(sizeof(float) * N);
  srand(1);
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < F; ++j) xs[i * F + j] = (float)rand() / RAND_MAX;
    ys[i] = xs[i * F] > 0.6f ? 1.f : 0.f;
  }
  flexmi_tensor_t label = flexmi_model_get_label_tensor(m);
  flexmi_dataloader_t dx = flexmi_single_dataloader_create(m, x, xs, N, 40);
  flexmi_dataloader_t dy = flexmi_single_dataloader_create(m, label, ys, N, 40);
  CHECK(dx && dy);
  for (int e = 0; e < 4; ++e) {
    flexmi_dataloader_reset(dx);
    flexmi_dataloader_reset(dy);
    flexmi_model_reset_metrics(m);
    for (int it = 0; it < N / B; ++it) {
      CHECK(flexmi_dataloader_next_batch(dx, m) == 0 && flexmi_dataloader_next_batch(dy, m) == 0);
      CHECK(flexmi_model_forward(m) == 0 && flexmi_model_zero_gradients(m) == 0);
      CHECK(flexmi_model_backward(m) == 0 && flexmi_model_update(m) == 0);
    }
  }
  flexmi_perf_metrics_t pm = flexmi_model_get_perf_metrics(m);
  CHECK(pm);
  printf("auc %.6f bound %.3e accuracy %.2f\n", flexmi_perf_metrics_get_auc(pm), flexmi_perf_metrics_get_auc_bound(pm),
         flexmi_perf_metrics_get_accuracy(pm));
  flexmi_perf_metrics_destroy(pm);
  flexmi_finalize();
  return 0;
}
"""


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs a C compiler")
def test_capi_reports_auc(tmp_path):
    lib = os.path.join(ROOT, "flexmi", "libflexmi_c.so")
    if not os.path.exists(lib):
        pytest.skip("libflexmi_c.so is not built")
    src, exe = str(tmp_path / "auc_c.c"), str(tmp_path / "auc_c")
    open(src, "w").write(C_PROG)
    subprocess.run(["gcc", src, f"-I{ROOT}/csrc/capi", f"-L{ROOT}/flexmi", "-lflexmi_c", f"-Wl,-rpath,{ROOT}/flexmi",
                    "-o", exe], check=True)
    r = subprocess.run([exe, "-b", "32", "--device", "cpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    auc = float(r.stdout.split("auc")[1].split()[0])
    bound = float(r.stdout.split("bound")[1].split()[0])
    assert 0.5 < auc <= 1.0 and 0.0 <= bound < 1e-2, r.stdout


# ------------------------------------------------------------------ 10. apps/dlrm.py
def _criteo_like(n, tables, seed):
    rng = np.random.RandomState(seed)
    return {"X_int": np.log(rng.randint(0, 1000, (n, 13)).astype(np.float32) + 1),
            "X_cat": np.concatenate([rng.randint(0, r, (n, 1)) for r in tables], 1).astype(np.int64),
            "y": rng.randint(0, 2, n).astype(np.float32)}


def _app():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dlrm_app_auc", os.path.join(ROOT, "apps", "dlrm.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


ARCH = ["--arch-sparse-feature-size", "8", "--arch-embedding-size", "30-40-50", "--arch-mlp-bot", "13-16-8",
        "--arch-mlp-top", "32-8-1", "-b", "64", "--device", "cpu"]


def test_dlrm_app_eval_pass_and_auc_threshold(tmp_path, native, capsys):
    from flexmi.utils.hdf5 import write_h5
    train, held = str(tmp_path / "train.h5"), str(tmp_path / "eval.h5")
    write_h5(train, _criteo_like(256, [30, 40, 50], 0))
    write_h5(held, _criteo_like(200, [30, 40, 50], 1))
    res = _app().main(ARCH + ["--dataset", train, "--eval-dataset", held, "--auc-threshold", "0.0", "-e", "3"])
    sps, met = res                                              # callers that unpack two values keep working
    out, err = capsys.readouterr()
    evals = [ln for ln in out.splitlines() if ln.startswith("EVAL epoch")]
    assert len(evals) == 1 and evals[0].startswith("EVAL epoch 0: loss "), out      # stopped after epoch 0
    assert re.fullmatch(r"EVAL epoch 0: loss \d+\.\d{5} accuracy \d+\.\d\d% auc \d\.\d{5} \(\+-\d\.\de-?\d\d\)", evals[0])
    assert met.eval is not None and met.eval.auc_pos + met.eval.auc_neg == 192 == met.eval.train_all   # 3 whole batches of 200
    assert 0.0 <= met.eval.get_auc() <= 1.0
    assert met.train_all == 256 and met.auc_pos + met.auc_neg == 256 and "1 epoch(s)" in err and " auc " in err
    # --eval-data-size caps the pass; without a threshold every epoch runs and evaluates
    _, met = _app().main(ARCH + ["--dataset", train, "--eval-dataset", held, "--eval-data-size", "128", "-e", "2"])
    out, err = capsys.readouterr()
    assert [ln[:12] for ln in out.splitlines() if ln.startswith("EVAL")] == ["EVAL epoch 0", "EVAL epoch 1"]
    assert met.eval.auc_pos + met.eval.auc_neg == 128 and "2 epoch(s)" in err


def test_dlrm_app_without_new_flags_prints_as_before(tmp_path, native, capsys):
    from flexmi.utils.hdf5 import write_h5
    train = str(tmp_path / "train.h5")
    write_h5(train, _criteo_like(256, [30, 40, 50], 0))
    sps, met = _app().main(ARCH + ["--dataset", train, "--data-size", "192", "-e", "2"])
    out, err = capsys.readouterr()
    assert met.eval is None and not met.has_auc and met.train_all == 192
    assert re.fullmatch(r"ELAPSED TIME = \d+\.\d{4}s, THROUGHPUT = \d+\.\d\d samples/s\n", out), out
    lines = [ln for ln in err.splitlines() if ln.startswith("[dlrm")]
    assert lines == [f"[dlrm custom] 2 epoch(s) x 3 iterations, batch 64, 1 device(s), dataset {train}: "
                     f"loss {met.get_loss():.5f} accuracy {met.get_accuracy():.2f}%"] or (
        len(lines) == 1 and re.fullmatch(r"\[dlrm \S+\] 2 epoch\(s\) x 3 iterations, batch 64, 1 device\(s\), dataset "
                                         + re.escape(train) + r": loss \d+\.\d{5} accuracy \d+\.\d\d%", lines[0])), err
    # --auc alone: the metric on the training metrics and the final line, no evaluation pass
    _, met = _app().main(ARCH + ["--dataset", train, "--auc", "-e", "1"])
    out, err = capsys.readouterr()
    assert met.has_auc and met.eval is None and met.auc_pos + met.auc_neg == 256 and "EVAL" not in out
    assert f" auc {met.get_auc():.5f} (+-{met.get_auc_bound():.1e})" in err
