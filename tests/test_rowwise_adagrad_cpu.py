"""RowwiseAdagradOptimizer on the CPU executor: the tiny DLRM against a plain-torch dense reference
(dense table gradient by ``index_add_``, the row-wise rule on ALL table rows, element-wise Adagrad
on dense parameters), the accumulator's size and checkpoint round trip, the placements rejected at
compile, the search's pricing and the command line."""
import json

import numpy as np
import pytest
import torch

from flexmi.core import (AdagradOptimizer, AggrMode, DataType, FFConfig, FFModel, LossType, MetricsType,
                         RowwiseAdagradOptimizer, SGDOptimizer)
from flexmi.core.types import OperatorType
from flexmi.ops.embedding import TableRule

B = 64
LR, EPS, H0 = 0.05, 1e-10, 0.1


def _cfg(batch=B):
    c = FFConfig()
    c.batchSize, c.device, c.compute_dtype = batch, "cpu", "fp32"
    return c


def _dlrm(opt_kw=None):
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    dcfg = DLRMConfig.preset("tiny")
    m = FFModel(_cfg())
    d, s, _ = build_dlrm(m, dcfg)
    kw = dict(lr=LR, initial_accumulator_value=H0)
    kw.update(opt_kw or {})
    m.compile(RowwiseAdagradOptimizer(m, **kw), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    return m, d, s, dcfg


def _batch(dcfg, it):
    rng = np.random.RandomState(3 + it)
    dense = rng.rand(B, 13).astype(np.float32)
    sp = [rng.randint(0, r, (B, 1)) for r in dcfg.embedding_size]     # 64 lookups of 30..200 rows: duplicates
    lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
    return dense, sp, lab


def _train(m, d, s, dcfg, steps, first=0):
    ex = m._ex()
    for it in range(first, first + steps):
        dense, sp, lab = _batch(dcfg, it)
        ex.scatter_from_host(d, dense)
        for t, a in zip(s, sp):
            ex.scatter_from_host(t, a)
        ex.scatter_from_host(m.get_label_tensor(), lab)
        ex.train_step()


def _params(m):
    return [torch.tensor(p.get_weights(m)) for p in m.parameters]


def _tables(m):
    ex = m._ex()
    return [ex.wentries[op.weights[0].guid] for op in m.layers if op.op_type == OperatorType.OP_EMBEDDING]


def _torch_dlrm(dense_ps, rows, x, F, bot_n, top_n):
    """Pure-PyTorch tiny DLRM (dot interaction) on the dense parameters and the looked-up rows."""
    i = 0
    for _ in range(bot_n):
        x = torch.relu(x @ dense_ps[i].t() + dense_ps[i + 1])
        i += 2
    Z = torch.stack([x] + rows, 1)
    G = Z @ Z.transpose(1, 2)
    li, lj = np.tril_indices(F, -1)
    z = torch.cat([x, G[:, li, lj]], 1)
    pad = dense_ps[i].shape[1] - z.shape[1]
    if pad:
        z = torch.cat([z, torch.zeros(z.shape[0], pad)], 1)
    for k in range(top_n):
        z = z @ dense_ps[i].t() + dense_ps[i + 1]
        z = torch.sigmoid(z) if k == top_n - 1 else torch.relu(z)
        i += 2
    return z


def test_tiny_dlrm_matches_dense_torch_reference():
    m, d, s, dcfg = _dlrm()
    m.init_layers()
    nb, nt = len(dcfg.mlp_bot) - 1, len(dcfg.mlp_top) - 1
    T = len(dcfg.embedding_size)
    tabs = _tables(m)
    assert len(tabs) == T
    for e, r in zip(tabs, dcfg.embedding_size):
        assert e.sparse and e.grad is None and e.group is None
        assert set(e.state) == {"h"} and tuple(e.state["h"].shape) == (r, 1)
        assert float(e.state["h"].min()) == float(e.state["h"].max()) == pytest.approx(H0)
        assert e.op.rule == TableRule("rowwise", EPS, None)
    # parameters in builder order: bottom linears, tables, top linears
    ps = _params(m)
    dense_ps = [p.clone().requires_grad_(True) for p in ps[:2 * nb] + ps[2 * nb + T:]]
    tables = [p.clone() for p in ps[2 * nb:2 * nb + T]]
    dense_h = [torch.full_like(p, H0) for p in dense_ps]
    table_h = [torch.full((t.shape[0],), H0) for t in tables]
    steps = 4
    _train(m, d, s, dcfg, steps)
    touched = [torch.zeros(t.shape[0], dtype=torch.bool) for t in tables]
    for it in range(steps):
        dense, sp, lab = _batch(dcfg, it)
        idx = [torch.tensor(a).view(-1) for a in sp]
        rows = [t[i].clone().requires_grad_(True) for t, i in zip(tables, idx)]
        out = _torch_dlrm(dense_ps, rows, torch.tensor(dense), T + 1, nb, nt)
        L = torch.nn.functional.binary_cross_entropy(out, torch.tensor(lab))
        g = torch.autograd.grad(L, dense_ps + rows)
        with torch.no_grad():
            for p, h, gg in zip(dense_ps, dense_h, g[:len(dense_ps)]):      # element-wise Adagrad
                h.addcmul_(gg, gg)
                p -= LR * gg / (h.sqrt() + EPS)
            for t, h, i, gr in zip(tables, table_h, idx, g[len(dense_ps):]):
                G = torch.zeros_like(t).index_add_(0, i, gr)                # the dense table gradient
                h += (G * G).mean(1)                                        # all rows: untouched ones add 0
                t -= LR * G / (h.sqrt() + EPS).unsqueeze(1)
        for tch, i in zip(touched, idx):
            tch[i] = True
    ref = [p.detach() for p in dense_ps[:2 * nb]] + tables + [p.detach() for p in dense_ps[2 * nb:]]
    for a, b in zip(_params(m), ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    for e, h, tch in zip(tabs, table_h, touched):
        torch.testing.assert_close(e.state["h"].view(-1), h, rtol=1e-5, atol=1e-6)
        assert bool((e.state["h"].view(-1)[~tch] == np.float32(H0)).all()) and int(tch.sum()) > 0
    assert any(int(tch.sum()) < tch.numel() for tch in touched)       # the inputs leave rows untouched
    rep = m._ex().memory_report()
    assert rep["sparse_opt_state"] == 4 * sum(dcfg.embedding_size)
    assert rep["sparse_tables"] == 4 * sum(dcfg.embedding_size) * dcfg.sparse_feature_size


def test_optimizer_interface():
    o = RowwiseAdagradOptimizer(None, 0.02, 1e-9, 0.0, 0.3)
    assert isinstance(o, AdagradOptimizer)
    assert o.state_names() == ["h"] and o.state_init("h") == 0.3
    assert o.sparse_capable and o.sparse_dp_capable
    assert not AdagradOptimizer(None).sparse_dp_capable          # the element-wise form is unchanged
    assert o.table_state_bytes(1000, 128) == 4000.0
    # dense parameters: AdagradOptimizer's rule
    w, g = torch.ones(4), torch.full((4,), 2.0)
    st = {"h": torch.full((4,), 0.3)}
    o.update_torch(w, g, st)
    torch.testing.assert_close(st["h"], torch.full((4,), 4.3))
    torch.testing.assert_close(w, torch.full((4,), 1 - 0.02 * 2 / (4.3 ** 0.5 + 1e-9)))


def test_checkpoint_round_trips_the_row_accumulators(tmp_path):
    ref, d, s, dcfg = _dlrm()
    ref.init_layers()
    _train(ref, d, s, dcfg, 3)
    a, d, s, _ = _dlrm()
    a.init_layers()
    _train(a, d, s, dcfg, 2)
    ck = str(tmp_path / "ck")
    a.save_checkpoint(ck)
    man = json.load(open(tmp_path / "ck" / "manifest.json"))
    assert man["optimizer"]["type"] == "RowwiseAdagradOptimizer"
    b, d, s, _ = _dlrm()
    b.init_layers()
    b.load_checkpoint(ck)
    for x, y in zip(_tables(a), _tables(b)):
        assert tuple(y.state["h"].shape) == (y.shape[0], 1) and torch.equal(x.state["h"], y.state["h"])
        assert float(y.state["h"].max()) > H0                    # the accumulator has moved and was restored
    _train(b, d, s, dcfg, 1, first=2)
    for p, q in zip(_params(b), _params(ref)):
        assert torch.equal(p, q)


# ------------------------------------------------------------------ rejected at compile
def _table_model(opt, strategy=None):
    m = FFModel(_cfg(16))
    idx = m.create_tensor([16, 1], DataType.DT_INT64)
    m.softmax(m.dense(m.embedding(idx, 12, 8, AggrMode.AGGR_MODE_SUM, name="mytable"), 4))
    if strategy:
        m.strategies = {"mytable": strategy}
    m.compile(opt(m), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    if strategy:
        m.strategies = {"mytable": strategy}
    return m


def test_host_placed_table_is_rejected():
    from flexmi.parallel.layout import ParallelConfig
    m = _table_model(lambda m: RowwiseAdagradOptimizer(m, 0.05), ParallelConfig([1, 1], [0], ParallelConfig.CPU))
    with pytest.raises(NotImplementedError, match="mytable.*host-placed"):
        m.init_layers()


def test_weight_decay_with_a_table_is_rejected():
    m = _table_model(lambda m: RowwiseAdagradOptimizer(m, 0.05, weight_decay=0.01))
    with pytest.raises(NotImplementedError, match="mytable.*weight_decay"):
        m.init_layers()
    # without a table weight decay is Adagrad's
    m = FFModel(_cfg(16))
    x = m.create_tensor([16, 6])
    m.softmax(m.dense(x, 4))
    m.compile(RowwiseAdagradOptimizer(m, 0.05, weight_decay=0.01), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY])
    m.init_layers()


def test_column_split_and_dense_replicas_are_rejected(monkeypatch):
    """The compile-time check on placements one process cannot hold (the two-rank compile of a column
    split is in test_rowwise_adagrad_distributed_cpu.py)."""
    from flexmi.parallel.layout import ParallelConfig
    from flexmi.runtime import executor as E
    m = _table_model(lambda m: RowwiseAdagradOptimizer(m, 0.05))
    ex = m.init_layers()
    op = m.layers[0]

    def check(pc):          # as Executor._build_weights does: the rule function, a reason raises
        lay = op.weight_layouts(pc)[0]
        rule, why = op.shard_rule(ex.optimizer, pc, lay, 0, lay.holders[0], sparse_dp=E.SPARSE_DP)
        if why:
            raise NotImplementedError(f"{op.name}: {why}")
        return rule
    assert check(ParallelConfig([1, 1], [0])) == TableRule("rowwise", EPS, None)
    assert check(ParallelConfig([1, 1, 2], [0, 1])) == TableRule("rowwise", EPS, None)
    cols2 = ParallelConfig([2, 1], [0, 1])
    with pytest.raises(NotImplementedError, match="mytable.*column-split"):
        check(cols2)
    dp2 = ParallelConfig([1, 2], [0, 1])
    assert op.weight_layouts(dp2)[0].replication() == 2
    assert check(dp2) == TableRule("rowwise", EPS, (0, 1))
    monkeypatch.setattr(E, "SPARSE_DP", False)
    with pytest.raises(NotImplementedError, match="mytable.*FLEXMI_SPARSE_DP"):
        check(dp2)


# ------------------------------------------------------------------ search and command line
def _big_table_model(opt_cls):
    m = FFModel(_cfg(64))
    idx = m.create_tensor([64, 1], DataType.DT_INT64)
    m.softmax(m.dense(m.embedding(idx, 100000, 16, AggrMode.AGGR_MODE_SUM), 4))
    m.optimizer = opt_cls(m, 0.05)
    return m


def test_search_pricing():
    from flexmi import cli
    from flexmi.parallel.layout import ParallelConfig
    from flexmi.parallel.search import SimGraph
    m = cli._model("dlrm-tiny", 2, 64, True, "rowwise_adagrad")
    assert isinstance(m.optimizer, RowwiseAdagradOptimizer)
    g = SimGraph(m, 2)
    gs = SimGraph(cli._model("dlrm-tiny", 2, 64, True, "sgd"), 2)
    from flexmi.ops.embedding import Embedding
    # sparse whether replicated or not, whatever the byte comparison says (4 rows: dense under SGD)
    assert Embedding.table_rule(m.optimizer, 4, 16, 32, (0,)) == (TableRule("rowwise", 1e-10, None), None)
    assert Embedding.table_rule(m.optimizer, 4, 16, 32, (0, 1)) == (TableRule("rowwise", 1e-10, (0, 1)), None)
    assert not Embedding.sdp_prefer_sparse(4, 16, 32, 2)
    n = dense_under_sgd = 0
    for k, op in enumerate(g.ops):
        if op.op_type != OperatorType.OP_EMBEDDING:
            continue
        n += 1
        assert g.cands[k] and all(op._grid(pc)[1] == 1 for pc in g.cands[k])          # no column split
        assert any(op._grid(pc)[1] > 1 for pc in gs.cands[k])                         # ... which SGD keeps
        assert [pc for pc in gs.cands[k] if op._grid(pc)[1] == 1] == g.cands[k]       # nothing else dropped
        # replicated (sample split over both devices): priced as the touched-row exchange although the
        # tiny table's dense all-reduce would move fewer bytes (SGD prices it dense)
        dp = ParallelConfig.data_parallel(op.out_ndims, 2)
        vol = op.num_entries * op.out_dim
        rec, rec_sgd = g._cand(op, dp), gs._cand(op, dp)
        payload = 4.0 * op.sdp_payload_words(32, op.out_dim)
        assert rec["wsync"] == [(2 * payload / 2.0, [0, 1])]
        if not Embedding.sdp_prefer_sparse(op.num_entries, op.out_dim, 32, 2):
            assert rec_sgd["wsync"] == [(float(vol * 4), [0, 1])] and vol * 4 < payload
            dense_under_sgd += 1
    assert n == 4 and dense_under_sgd == 1            # the 30-row table
    # whole-table placement: the state is one fp32 per row (element-wise Adagrad: per element)
    vol, rows = 100000 * 16, 100000
    mem = {}
    for name, cls in (("sgd", SGDOptimizer), ("adagrad", AdagradOptimizer), ("rowwise", RowwiseAdagradOptimizer)):
        g = SimGraph(_big_table_model(cls), 2)
        k = next(i for i, op in enumerate(g.ops) if op.op_type == OperatorType.OP_EMBEDDING)
        rec = g._cand(g.ops[k], ParallelConfig([1, 1], [0]))
        assert rec["wsync"] == []
        mem[name] = dict(rec["mem"])[0]
    assert mem["adagrad"] - mem["sgd"] == vol * 4.0
    assert mem["rowwise"] - mem["sgd"] == rows * 4.0


@pytest.mark.parametrize("cmd", ["simulate", "search"])
def test_cli_accepts_the_optimizer(capsys, cmd):
    from flexmi import cli
    extra = ["--budget", "20"] if cmd == "search" else []
    assert cli.main([cmd, "--model", "dlrm-tiny", "--small", "--gpus", "2", "--optimizer", "rowwise_adagrad"] + extra) == 0
    lines = [ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("{")]
    assert lines and json.loads(lines[-1])
