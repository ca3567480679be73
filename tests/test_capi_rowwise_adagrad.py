"""Row-wise Adagrad through the C API (csrc/capi/flexmi_c.h): tests/capi/rowwise_adagrad_emb.c
trains an MLP with an embedding bag for two steps on the CPU backend; the same model built through
the Python API ends with exactly the same parameters, and its table was trained row-wise."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flexmi", "libflexmi_c.so")


def _python_run():
    from flexmi.core import (ActiMode, AggrMode, DataType, FFConfig, FFModel, LossType, MetricsType,
                             RowwiseAdagradOptimizer, SingleDataLoader)
    B, F, C, N, ROWS, D, BAG = 16, 12, 4, 32, 20, 8, 2
    cfg = FFConfig()
    cfg.batchSize, cfg.device = B, "cpu"
    m = FFModel(cfg)
    x = m.create_tensor([B, F], name="input")
    idx = m.create_tensor([B, BAG], DataType.DT_INT32, name="indices")
    t = m.dense(x, D, ActiMode.AC_MODE_RELU, name="dense1")
    t = m.add(t, m.embedding(idx, ROWS, D, AggrMode.AGGR_MODE_SUM, name="table"), name="add")
    t = m.dense(t, C, name="dense2")
    t = m.softmax(t, name="softmax")
    opt = RowwiseAdagradOptimizer(m, 0.1, 1e-10, 0.0, 0.1)
    m.compile(opt, LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.init_layers()
    opt.set_learning_rate(0.05)
    i, j = np.meshgrid(np.arange(N), np.arange(F), indexing="ij")
    X = ((31 * i + 17 * j) % 97).astype(np.float32) / np.float32(97.0)
    Y = ((7 * np.arange(N)) % 4).astype(np.int32).reshape(N, 1)
    I = ((5 * np.arange(N)[:, None] + 3 * np.arange(BAG)[None, :]) % ROWS).astype(np.int32)
    dx = SingleDataLoader(m, x, X, N)
    dy = SingleDataLoader(m, m.get_label_tensor(), Y, N)
    di = SingleDataLoader(m, idx, I, N)
    for _ in range(2):
        dx.next_batch(m)
        dy.next_batch(m)
        di.next_batch(m)
        m.forward()
        m.zero_gradients()
        m.backward()
        m.update()
    table = next(e for e in m._ex().wentries.values() if e.sparse)
    assert set(table.state) == {"h"} and tuple(table.state["h"].shape) == (ROWS, 1)
    assert float(table.state["h"].max()) > 0.1
    return [p.get_weights(m).reshape(-1) for p in m.parameters]


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs a C compiler")
def test_c_rowwise_adagrad_equals_python(tmp_path):
    assert os.path.exists(LIB), "build the C API first (tools/build_ext.py)"
    hdr = open(os.path.join(ROOT, "csrc", "capi", "flexmi_c.h")).read()
    for name in ("flexmi_rowwise_adagrad_optimizer_create(", "flexmi_model_set_adagrad_optimizer(",
                 "flexmi_optimizer_set_lr(", "flexmi_optimizer_destroy("):
        assert name in hdr
    exe = str(tmp_path / "rowwise_adagrad_emb")
    subprocess.run(["gcc", os.path.join(ROOT, "tests", "capi", "rowwise_adagrad_emb.c"), f"-I{ROOT}/csrc/capi",
                    f"-L{ROOT}/flexmi", "-lflexmi_c", f"-Wl,-rpath,{ROOT}/flexmi", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("param "):
            f = ln.split()
            got[int(f[1])] = np.array([float(v) for v in f[3:]], dtype=np.float32)
            assert got[int(f[1])].size == int(f[2])
    ref = _python_run()
    assert len(ref) == 5 and sorted(got) == [0, 1, 2, 3, 4]
    for k, a in enumerate(ref):
        assert np.array_equal(got[k], a), (k, np.abs(got[k] - a).max())
