"""AdagradOptimizer on the CPU executor: against ``torch.optim.Adagrad`` (dense parameters and a
sparsely updated embedding table with duplicate lookups), weight decay (tables fall back to the
dense path), ZeRO-1, checkpoint / resume, the Keras front end and the search's pricing."""
import json
import os

import numpy as np
import pytest
import torch

from flexmi.core import (ActiMode, AdagradOptimizer, AggrMode, DataType, FFConfig, FFModel, LossType, MetricsType,
                         SGDOptimizer)

B, ROWS, D, BAG = 16, 12, 8, 3


def _cfg(zero=0):
    c = FFConfig()
    c.batchSize, c.device, c.compute_dtype = B, "cpu", "fp32"
    if zero:
        c.zero_stage, c.grad_bucket_mb = zero, 0.002
    return c


def _model(opt_kw, table=True, zero=0):
    """x -> dense(D, relu) [+ EmbeddingBag(sum)] -> dense(4) -> softmax."""
    m = FFModel(_cfg(zero))
    x = m.create_tensor([B, 10])
    t = m.dense(x, D, ActiMode.AC_MODE_RELU)
    idx = None
    if table:
        idx = m.create_tensor([B, BAG], DataType.DT_INT64)
        t = m.add(t, m.embedding(idx, ROWS, D, AggrMode.AGGR_MODE_SUM))
    t = m.softmax(m.dense(t, 4))
    m.compile(AdagradOptimizer(m, **opt_kw), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY])
    m.init_layers()
    return m, x, idx


def _batch(step, table=True):
    rng = np.random.RandomState(10 + step)
    X = rng.randn(B, 10).astype(np.float32)
    # 12 rows, 48 lookups per step: every step has duplicates inside bags and across samples
    I = rng.randint(0, ROWS, (B, BAG)).astype(np.int64)
    I[:, 1] = I[:, 0]
    Y = rng.randint(0, 4, (B, 1)).astype(np.int32)
    return X, I, Y


def _train(m, x, idx, steps, first=0):
    ex = m._ex()
    for s in range(first, first + steps):
        X, I, Y = _batch(s)
        ex.scatter_from_host(x, X)
        if idx is not None:
            ex.scatter_from_host(idx, I)
        ex.scatter_from_host(m.get_label_tensor(), Y)
        ex.train_step()


def _params(m):
    return [torch.tensor(p.get_weights(m)) for p in m.parameters]


def _torch_run(ps, table, steps, **kw):
    ps = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adagrad(ps, **kw)
    for s in range(steps):
        X, I, Y = _batch(s)
        h = torch.relu(torch.tensor(X) @ ps[0].t() + ps[1])
        if table:
            h = h + torch.nn.functional.embedding_bag(torch.tensor(I), ps[2], mode="sum")
            w, b = ps[3], ps[4]
        else:
            w, b = ps[2], ps[3]
        out = torch.log_softmax(h @ w.t() + b, -1)
        loss = torch.nn.functional.nll_loss(out, torch.tensor(Y).long().view(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return [p.detach() for p in ps]


def _table_entry(m):
    return next(e for e in m._ex().wentries.values() if tuple(e.shape) == (ROWS, D) and e.op.op_type.name == "OP_EMBEDDING")


@pytest.mark.parametrize("h0", [0.0, 0.1])
def test_sparse_table_and_mlp_match_torch(h0):
    m, x, idx = _model(dict(lr=0.05, initial_accumulator_value=h0))
    e = _table_entry(m)
    assert e.sparse and e.grad is None and set(e.state) == {"h"}
    assert float(e.state["h"].min()) == float(e.state["h"].max()) == pytest.approx(h0)
    start = _params(m)
    _train(m, x, idx, 3)
    ref = _torch_run(start, True, 3, lr=0.05, initial_accumulator_value=h0, eps=1e-10)
    for a, b in zip(_params(m), ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    rep = m._ex().memory_report()
    assert rep["sparse_opt_state"] == ROWS * D * 4 and rep["sparse_tables"] == ROWS * D * 4


def test_dense_mlp_with_weight_decay_matches_torch():
    m, x, _ = _model(dict(lr=0.05, weight_decay=0.01, initial_accumulator_value=0.1), table=False)
    start = _params(m)
    _train(m, x, None, 3)
    ref = _torch_run(start, False, 3, lr=0.05, weight_decay=0.01, initial_accumulator_value=0.1, eps=1e-10)
    for a, b in zip(_params(m), ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_weight_decay_keeps_tables_dense():
    opt = AdagradOptimizer(None, 0.05, weight_decay=0.01)
    assert not opt.sparse_capable and not opt.sparse_dp_capable
    assert AdagradOptimizer(None).sparse_capable and not AdagradOptimizer(None).sparse_dp_capable
    assert SGDOptimizer(None, 0.1).sparse_dp_capable and not SGDOptimizer(None, 0.1, momentum=0.9).sparse_dp_capable
    m, x, idx = _model(dict(lr=0.05, weight_decay=0.01, initial_accumulator_value=0.1))
    e = _table_entry(m)
    assert not e.sparse and e.grad is not None and e.group is not None
    start = _params(m)
    _train(m, x, idx, 3)
    ref = _torch_run(start, True, 3, lr=0.05, weight_decay=0.01, initial_accumulator_value=0.1, eps=1e-10)
    for a, b in zip(_params(m), ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_optimizer_interface():
    o = AdagradOptimizer(None, 0.02, 1e-9, 0.0, 0.3)
    assert o.state_names() == ["h"] and o.state_init("h") == 0.3
    assert SGDOptimizer(None, 0.1, momentum=0.9).state_init("v") == 0.0
    w, g = torch.ones(4), torch.full((4,), 2.0)
    st = {"h": torch.full((4,), 0.3)}
    o.update_torch(w, g, st)
    torch.testing.assert_close(st["h"], torch.full((4,), 4.3))
    torch.testing.assert_close(w, torch.full((4,), 1 - 0.02 * 2 / (4.3 ** 0.5 + 1e-9)))
    o.load_state_dict({"lr": 0.5})
    assert o.state_dict() == {"lr": 0.5}


def test_set_learning_rate_reaches_the_executor():
    m, x, idx = _model(dict(lr=0.05))
    m.optimizer.set_learning_rate(0.25)
    assert float(m._ex().lr_tensor[0]) == 0.25


def test_zero1_world1_equals_plain():
    kw = dict(lr=0.05, initial_accumulator_value=0.1)
    m0, x0, i0 = _model(kw)
    m1, x1, i1 = _model(kw, zero=1)
    _train(m0, x0, i0, 3)
    _train(m1, x1, i1, 3)
    for a, b in zip(_params(m0), _params(m1)):
        assert torch.equal(a, b)


def test_checkpoint_resume_is_exact(tmp_path):
    kw = dict(lr=0.05, initial_accumulator_value=0.1)
    ref, x, idx = _model(kw)
    _train(ref, x, idx, 3)
    a, x, idx = _model(kw)
    _train(a, x, idx, 2)
    ck = str(tmp_path / "ck")
    a.save_checkpoint(ck)
    man = json.load(open(os.path.join(ck, "manifest.json")))
    assert man["optimizer"]["type"] == "AdagradOptimizer"
    b, x, idx = _model(kw)
    b.load_checkpoint(ck)
    assert torch.equal(_table_entry(b).state["h"], _table_entry(a).state["h"])
    assert float(_table_entry(b).state["h"].max()) > 0.1      # the accumulator has moved and was restored
    _train(b, x, idx, 1, first=2)
    for p, q in zip(_params(b), _params(ref)):
        assert torch.equal(p, q)


def test_host_placed_table_is_rejected():
    from flexmi.parallel.layout import ParallelConfig
    m = FFModel(_cfg())
    idx = m.create_tensor([B, 1], DataType.DT_INT64)
    e = m.embedding(idx, ROWS, D, AggrMode.AGGR_MODE_SUM)
    t = m.softmax(m.dense(e, 4))
    m.strategies = {m.layers[0].name: ParallelConfig([1, 1], [0], ParallelConfig.CPU)}
    m.compile(AdagradOptimizer(m, 0.05), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.strategies = {m.layers[0].name: ParallelConfig([1, 1], [0], ParallelConfig.CPU)}
    with pytest.raises(NotImplementedError):
        m.init_layers()


def test_keras_adagrad_trains():
    from flexmi.keras import layers, models, optimizers
    o = optimizers.Adagrad()
    assert (o.lr, o.h0, o.eps) == (0.001, 0.1, 1e-7)
    rng = np.random.RandomState(0)
    X = rng.randn(128, 12).astype(np.float32)
    Y = (X[:, :4].argmax(1)).astype(np.int32).reshape(-1, 1)
    cfg = _cfg()
    cfg.batchSize = 32
    inp = layers.Input(shape=(12,))
    t = layers.Dense(32, activation="relu")(inp)
    out = layers.Activation("softmax")(layers.Dense(4)(t))
    model = models.Model(inp, out, ffconfig=cfg)
    model.compile(optimizers.Adagrad(learning_rate=0.1), loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    assert isinstance(model.ffmodel.optimizer, AdagradOptimizer)
    assert model.ffmodel.optimizer.initial_accumulator_value == 0.1 and model.ffmodel.optimizer.epsilon == 1e-7
    m, ex = model.ffmodel, model.ffmodel._ex()
    x_t = model._inputs[0].ff
    losses_seen = []
    for ep in range(6):
        m.reset_metrics()
        for k in range(0, 128, 32):
            ex.scatter_from_host(x_t, X[k:k + 32])
            ex.scatter_from_host(m.get_label_tensor(), Y[k:k + 32])
            ex.train_step()
        losses_seen.append(m.get_perf_metrics().get_loss())
    assert losses_seen[-1] < losses_seen[0]


def _big_table_model(opt_cls):
    cfg = _cfg()
    cfg.batchSize = 64
    m = FFModel(cfg)
    idx = m.create_tensor([64, 1], DataType.DT_INT64)
    t = m.softmax(m.dense(m.embedding(idx, 100000, 16, AggrMode.AGGR_MODE_SUM), 4))
    m.optimizer = opt_cls(m, 0.05)
    return m


def _dp_record(graph, op_index, ndev):
    from flexmi.parallel.layout import ParallelConfig
    op = graph.ops[op_index]
    dp = ParallelConfig.data_parallel(op.out_ndims, ndev)
    assert dp in graph.cands[op_index]
    return graph._cand(op, dp)


def test_search_prices_replicated_tables_dense(capsys):
    from flexmi import cli
    from flexmi.parallel.search import SimGraph
    assert cli.main(["search", "--model", "dlrm-tiny", "--small", "--gpus", "2", "--budget", "20",
                     "--optimizer", "adagrad"]) == 0
    rec = json.loads([ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("{")][-1])
    assert rec["best_ms"] > 0
    m = cli._model("dlrm-tiny", 2, 64, True, "adagrad")
    assert isinstance(m.optimizer, AdagradOptimizer)
    g = SimGraph(m, 2)
    from flexmi.ops.embedding import Embedding, TableRule
    # sparse where the table is not replicated, dense where it is -- even where SGD would go sparse
    assert Embedding.table_rule(m.optimizer, 100000, 16, 32, (0,)) == (TableRule("adagrad", 1e-10, None), None)
    assert Embedding.table_rule(m.optimizer, 100000, 16, 32, (0, 1)) == (None, None)
    assert Embedding.sdp_prefer_sparse(100000, 16, 32, 2)
    n = 0
    for k, op in enumerate(g.ops):
        if op.op_type.name != "OP_EMBEDDING":
            continue
        rec = _dp_record(g, k, 2)          # sample split = the table replicated on both devices
        vol = op.num_entries * op.out_dim
        assert rec["wsync"] == [(float(vol * 4), [0, 1])]
        # master + gradient + bf16 mirror + h, beside the activations
        assert dict(rec["mem"])[0] >= vol * (4.0 + 4.0 + 2.0 + 4.0)
        n += 1
    assert n == 4
    # a table big enough for SGD to prefer sparse data parallelism: Adagrad still prices it dense,
    # and a whole-table placement carries one extra table-sized state buffer
    from flexmi.parallel.layout import ParallelConfig
    vol = 100000 * 16
    recs = {}
    for name, cls in (("sgd", SGDOptimizer), ("adagrad", AdagradOptimizer)):
        g = SimGraph(_big_table_model(cls), 2)
        k = next(i for i, op in enumerate(g.ops) if op.op_type.name == "OP_EMBEDDING")
        one = g._cand(g.ops[k], ParallelConfig([1, 1], [0]))
        recs[name] = (_dp_record(g, k, 2), one)
    assert recs["sgd"][0]["wsync"][0][0] < vol * 4.0            # touched-row all-gather
    assert recs["adagrad"][0]["wsync"] == [(float(vol * 4), [0, 1])]
    assert recs["adagrad"][1]["wsync"] == [] and recs["sgd"][1]["wsync"] == []
    assert dict(recs["adagrad"][1]["mem"])[0] - dict(recs["sgd"][1]["mem"])[0] == vol * 4.0
