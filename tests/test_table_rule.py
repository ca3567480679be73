"""How an embedding table is trained is decided in one place, ``Embedding.table_rule``: its outcome
table, and that the executor (``Executor._build_weights``) and the strategy search
(``SimGraph._cand``) both follow it -- what the executor allocates per table equals what the search
priced for the same placement."""
import os
import socket
import sys

import pytest
import torch.multiprocessing as mp

from flexmi.core import AdagradOptimizer, AdamOptimizer, RowwiseAdagradOptimizer, SGDOptimizer
from flexmi.ops.embedding import Embedding, TableRule

EPS = 1e-9
OPTS = {
    "none": lambda: None,
    "adam": lambda: AdamOptimizer(None),
    "sgd": lambda: SGDOptimizer(None, 0.1),
    "sgd_momentum": lambda: SGDOptimizer(None, 0.1, momentum=0.9),
    "sgd_wd": lambda: SGDOptimizer(None, 0.1, weight_decay=0.01),
    "adagrad": lambda: AdagradOptimizer(None, 0.1, EPS),
    "adagrad_wd": lambda: AdagradOptimizer(None, 0.1, EPS, weight_decay=0.01),
    "rowwise": lambda: RowwiseAdagradOptimizer(None, 0.1, EPS),
    "rowwise_wd": lambda: RowwiseAdagradOptimizer(None, 0.1, EPS, weight_decay=0.01),
}
# (rows, D, lookups per replica): at R = 2 the sparse all-gather wins / the dense all-reduce wins
SHAPES = {"big": (100000, 16, 32), "small": (4, 16, 32)}
HOST_SGD_ONLY = "CPU placement is supported for embedding tables trained with SGD"


def _expected(name, R, host, colsplit, sdp, shape):
    """(rule, fragment of the rejection message) by the outcome table, written out case by case."""
    reps = tuple(range(R)) if R > 1 else None
    if name.startswith("rowwise"):
        if host:
            return None, "host-placed"
        if colsplit:
            return None, "column-split"
        if name == "rowwise_wd":
            return None, "weight_decay"
        if R > 1 and not sdp:
            return None, "FLEXMI_SPARSE_DP"
        return TableRule("rowwise", EPS, reps), None
    if name == "sgd":
        if host:
            return TableRule("sgd", None, None, True), None
        if R == 1:
            return TableRule("sgd"), None
        return (TableRule("sgd", None, reps) if sdp and Embedding.sdp_prefer_sparse(*shape, R) else None), None
    if host:
        return None, HOST_SGD_ONLY
    if name == "adagrad" and R == 1:
        return TableRule("adagrad", EPS), None
    return None, None      # no optimizer, Adam, SGD with momentum / weight decay, Adagrad with weight decay or replicated


def test_the_two_shapes_straddle_the_byte_comparison():
    assert Embedding.sdp_prefer_sparse(*SHAPES["big"], 2) and not Embedding.sdp_prefer_sparse(*SHAPES["small"], 2)


@pytest.mark.parametrize("sdp", [True, False])
@pytest.mark.parametrize("colsplit", [False, True])
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(OPTS))
def test_rule_table(name, shape, R, host, colsplit, sdp):
    rows, D, lookups = SHAPES[shape]
    rule, why = Embedding.table_rule(OPTS[name](), rows, D, lookups, tuple(range(R)), host=host, colsplit=colsplit,
                                     sparse_dp=sdp)
    exp, frag = _expected(name, R, host, colsplit, sdp, SHAPES[shape])
    assert rule == exp
    if frag is None:
        assert why is None
    else:
        assert frag in why
        if name.startswith("rowwise"):
            assert why.startswith("row-wise Adagrad: ")
    if rule is not None:
        assert rule.state_shape(rows, D) == {"sgd": None, "adagrad": (rows, D), "rowwise": (rows, 1)}[rule.kind]


def test_rule_is_a_value():
    assert TableRule("rowwise", 1e-10) == TableRule("rowwise", 1e-10, None, False)
    assert TableRule("sgd", None, (0, 1)) != TableRule("sgd", None, (0, 2)) and TableRule("sgd") != TableRule("adagrad")
    assert hash(TableRule("sgd", None, (0, 1))) == hash(TableRule("sgd", None, (0, 1)))
    with pytest.raises(AttributeError):
        TableRule("sgd").kind = "adagrad"


# ------------------------------------------------------------------ executor and search agree
B, BAG, D = 16, 2, 8
ROWS = [4, 256, 4096]      # dense under replicated SGD; in between; rows well above the lookups
TRAIN = {"sgd": lambda m: SGDOptimizer(m, 0.05), "adagrad": lambda m: AdagradOptimizer(m, 0.05, EPS),
         "rowwise": lambda m: RowwiseAdagradOptimizer(m, 0.05, EPS)}


def _model(world, placement, opt):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, dlrm_strategy
    from flexmi.parallel.layout import ParallelConfig
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    build_dlrm(m, DLRMConfig(D, list(ROWS), [13, 16, D], [32, 16, 1], BAG, -1, -1, 0.0, "dot", "", -1, "bce", "rule"))
    strat = {}
    if placement == "rowsplit":     # tables whole on one rank each, one split by rows over both
        strat = dlrm_strategy(m, world, split_factor=1e9)
        strat["embedding2"] = ParallelConfig([1, 1, world], list(range(world)))
    m.strategies = strat
    m.compile(TRAIN[opt](m), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.strategies = strat
    return m


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _check(world, placement, opt):
    """This rank's executor against the search's record of every table, both against the rule."""
    from flexmi.core.types import OperatorType
    from flexmi.parallel.search import SimGraph
    m = _model(world, placement, opt)
    ex = m.init_layers()
    g = SimGraph(m, world)
    nstates = len(m.optimizer.state_names())
    seen = set()
    for op in m.layers:
        if op.op_type != OperatorType.OP_EMBEDDING:
            continue
        pc = ex.pcs[op.guid]
        rec = g._cand(op, pc)
        lay = op.weight_layouts(pc)[0]
        out = op.output_layouts(pc)[0]
        mem = {}
        for p, dev in enumerate(pc.device_ids):         # activations: output and its gradient
            mem[dev] = mem.get(dev, 0.0) + _prod(hi - lo for lo, hi in out.part_box(p)) * g.cost.eb * 2
        wsync = []
        for p in range(lay.num_parts()):
            h = lay.holders[p]
            R = len(h)
            (r0, r1), (c0, c1) = lay.part_box(p)
            rows, cols, vol = r1 - r0, c1 - c0, (r1 - r0) * (c1 - c0)
            lookups = -(-B // R) * BAG
            rule, why = Embedding.table_rule(m.optimizer, rows, cols, lookups, h)
            assert why is None
            seen.add((rule.kind if rule else "dense", R > 1))
            state = 4 * _prod(rule.state_shape(rows, cols) or (0,)) if rule else None
            words = 0
            if R > 1 and rule is not None:
                assert rule.replicas == tuple(sorted(h))
                words = R * (1 + lookups * (1 + cols))
                wsync.append((4.0 * words / 2.0, list(h)))
                if rule.kind == "rowwise":
                    words += min(rows, R * lookups) * (cols + 1)
            elif R > 1:
                wsync.append((float(vol * 4), list(h)))
            for d in h:
                mem[d] = mem.get(d, 0.0) + (vol * 4.0 + state + words * 4.0 if rule else vol * (10.0 + 4.0 * nstates))
            if ex.rank in h:                              # what the executor built for this shard
                e = ex.wentries[op.weights[0].guid]
                assert e.shape == (rows, cols) and e.holders == h
                assert op.rule == rule and e.sparse == (rule is not None)
                # a dense table's state lies in its sync group: one buffer of its shape per state name
                assert sum(t.numel() * 4 for t in e.state.values()) == (state if rule else vol * 4 * nstates)
                assert (e.group is None) == e.sparse
                if rule is not None and rule.kind != "sgd":
                    assert tuple(e.state["h"].shape) == rule.state_shape(rows, cols)
        assert rec["wsync"] == wsync, (op.name, rec["wsync"], wsync)
        assert dict(rec["mem"]) == mem, (op.name, rec["mem"], mem)
    return seen


EXPECT = {   # (how a table is trained, replicated) met per placement and optimizer
    ("w1", "sgd"): {("sgd", False)}, ("w1", "adagrad"): {("adagrad", False)}, ("w1", "rowwise"): {("rowwise", False)},
    ("dp", "sgd"): {("sgd", True), ("dense", True)}, ("dp", "adagrad"): {("dense", True)},
    ("dp", "rowwise"): {("rowwise", True)},
    ("rowsplit", "sgd"): {("sgd", False)}, ("rowsplit", "adagrad"): {("adagrad", False)},
    ("rowsplit", "rowwise"): {("rowwise", False)},
}


def _job(world, placement):
    for opt in sorted(TRAIN):
        assert _check(world, placement, opt) == EXPECT[(placement, opt)], (placement, opt)


def _worker(rank, world, port, placement):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rc = 0
    try:
        _job(world, placement)
    except BaseException:  # noqa: BLE001 -- reported through the exit code
        import traceback
        traceback.print_exc()
        rc = 1
    finally:
        dist.destroy_process_group()   # ordered teardown: normal interpreter exit afterwards
    sys.exit(rc)


def test_executor_and_search_agree_world1():
    _job(1, "w1")


@pytest.mark.multiproc
@pytest.mark.parametrize("placement", ["dp", "rowsplit"])
def test_executor_and_search_agree_world2(placement):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker, args=(2, port, placement), nprocs=2, join=True, start_method="spawn")
