"""Per-table multi-hot bag sizes for DLRM on the fp32 CPU executor: ``DLRMConfig.embedding_bag_sizes``
and its flag, the ``*_multihot`` presets and zoo names, ``tiny_dcn_multihot`` trained against a
plain-torch replica (SGD and row-wise Adagrad), the four tables running as ONE embedding group, and
the HDF5 data path reading table ``i`` from columns ``[off_i, off_i + bag_i)`` of ``X_cat``."""
import importlib.util
import os

import numpy as np
import pytest
import torch

BAGS = [3, 1, 8, 2]


def _cpu_model(B):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    return FFModel(cfg)


# ------------------------------------------------------------------ config, flag, presets, zoo
def test_flag_and_bag_sizes():
    from flexmi.models.dlrm import DLRMConfig
    c = DLRMConfig.parse_args(["dlrm", "--arch-embedding-size", "100-50-200-30", "--embedding-bag-sizes", "3-1-8-2"])
    assert c.embedding_bag_sizes == BAGS and c.bag_sizes() == BAGS
    s = DLRMConfig.parse_args(["dlrm", "--arch-embedding-size", "10-20-30", "--embedding-bag-size", "5"])
    assert s.embedding_bag_sizes == [] and s.bag_sizes() == [5, 5, 5]
    assert DLRMConfig().bag_sizes() == [1]
    # a later --embedding-bag-size clears the list; the flags may come in any order
    c = DLRMConfig.parse_args(["dlrm", "--embedding-bag-sizes", "3-1-8-2", "--embedding-bag-size", "4",
                               "--arch-embedding-size", "100-50-200-30"])
    assert c.embedding_bag_sizes == [] and c.bag_sizes() == [4] * 4
    c = DLRMConfig.parse_args(["dlrm", "--embedding-bag-size", "4", "--embedding-bag-sizes", "3-1-8-2"],
                              DLRMConfig.preset("tiny_dcn"))
    assert c.bag_sizes() == BAGS


@pytest.mark.parametrize("bags,lens", [([3, 1, 8], ("3", "4")), ([3, 1, 8, 2, 2], ("5", "4")), ([3, 0, 8, 2], ("4", "4"))])
def test_bad_bag_sizes_raise_at_build(bags, lens):
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    c = DLRMConfig.parse_args(["dlrm", "--embedding-bag-sizes", "-".join(map(str, bags))], DLRMConfig.preset("tiny_dcn"))
    assert c.embedding_bag_sizes == bags                        # parsing accepts it: build_dlrm rejects it
    with pytest.raises(ValueError) as e:
        build_dlrm(_cpu_model(8), c)
    assert f"{lens[0]} entries" in str(e.value) and f"{lens[1]} embedding tables" in str(e.value)


def test_presets_and_zoo():
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import MLPERF_MULTIHOT_SIZES, MLPERF_TABLES, DLRMConfig, build_dlrm
    from flexmi.models.zoo import build
    assert len(MLPERF_MULTIHOT_SIZES) == 26 and sum(MLPERF_MULTIHOT_SIZES) == 214
    assert min(MLPERF_MULTIHOT_SIZES) == 1 and max(MLPERF_MULTIHOT_SIZES) == 100
    c, one = DLRMConfig.preset("mlperf_dcnv2_multihot"), DLRMConfig.preset("mlperf_dcnv2")
    assert c.name == "mlperf_dcnv2_multihot" and c.bag_sizes() == MLPERF_MULTIHOT_SIZES
    assert one.embedding_bag_sizes == [] and one.bag_sizes() == [1] * 26
    assert (c.embedding_size, c.mlp_bot, c.mlp_top, c.arch_interaction_op, c.dcn_layers, c.dcn_rank) == (
        MLPERF_TABLES, one.mlp_bot, one.mlp_top, "dcn", 3, 512)
    t, t1 = DLRMConfig.preset("tiny_dcn_multihot"), DLRMConfig.preset("tiny_dcn")
    assert t.bag_sizes() == BAGS and (t.embedding_size, t.mlp_top) == (t1.embedding_size, t1.mlp_top)
    m = _cpu_model(8)
    _, sparse, _ = build_dlrm(m, c)                             # graph only: no table is allocated
    assert [tuple(s.dims) for s in sparse] == [(8, b) for b in MLPERF_MULTIHOT_SIZES]
    for name, bags in (("dlrm-tiny_dcn_multihot", BAGS), ("dlrm-mlperf_dcnv2_multihot", MLPERF_MULTIHOT_SIZES)):
        m = _cpu_model(16)
        built = build(name, m)
        embs = [op for op in m.layers if op.op_type == OperatorType.OP_EMBEDDING]
        assert [op.inputs[0].dims[1] for op in embs] == bags
        assert [tuple(built.inputs[f"sparse{i}"].dims) for i in range(len(bags))] == [(16, b) for b in bags]


def test_cli_simulate_takes_the_zoo_name(capsys):
    import json
    from flexmi import cli
    cli.main(["simulate", "--model", "dlrm-tiny_dcn_multihot", "--gpus", "2", "--batch", "64"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["model"] == "dlrm-tiny_dcn_multihot" and res["predicted_ms"] > 0


# ------------------------------------------------------------------ tiny_dcn_multihot against a torch replica
def _batches(dcfg, B, n):
    """n batches; batch 1 holds the same row twice in one bag of every multi-lookup table."""
    rng = np.random.RandomState(3)
    out = []
    for k in range(n):
        dense = rng.rand(B, 13).astype(np.float32)
        idx = [rng.randint(0, r, (B, b)).astype(np.int64) for r, b in zip(dcfg.embedding_size, dcfg.bag_sizes())]
        if k == 1:
            for a in idx:
                if a.shape[1] > 1:
                    a[2, -1] = a[2, 0]
        out.append((dense, idx, rng.randint(0, 2, (B, 1)).astype(np.float32)))
    return out


@pytest.mark.parametrize("optname", ["sgd", "rowwise_adagrad"])
def test_tiny_dcn_multihot_matches_torch_replica(optname):
    from flexmi.core import LossType, MetricsType, RowwiseAdagradOptimizer, SGDOptimizer
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    B, lr, eps = 16, 0.1, 1e-10
    dcfg = DLRMConfig.preset("tiny_dcn_multihot")
    m = _cpu_model(B)
    d, s, _ = build_dlrm(m, dcfg)
    assert [tuple(t.dims) for t in s] == [(16, 3), (16, 1), (16, 8), (16, 2)]
    opt = SGDOptimizer(m, lr) if optname == "sgd" else RowwiseAdagradOptimizer(m, lr, epsilon=eps)
    m.compile(opt, LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    W = [torch.tensor(p.get_weights(m), dtype=torch.float32, requires_grad=True) for p in m.parameters]
    names = [p.name for p in m.parameters]
    tables = {id(w) for w, p in zip(W, m.parameters) if p.owner_op.op_type == OperatorType.OP_EMBEDDING}
    assert len(tables) == 4
    H = [torch.zeros(w.shape[0], 1) if id(w) in tables else torch.zeros_like(w) for w in W]

    def replica(dense, idx):
        it = iter(W)
        lin = lambda x: torch.nn.functional.linear(x, next(it), next(it))
        x = torch.relu(lin(torch.relu(lin(dense))))            # bottom 13-32-16
        embs = [torch.nn.functional.embedding_bag(i, next(it), mode="sum") for i in idx]
        z0 = z = torch.cat([x] + embs, 1)
        for _ in range(dcfg.dcn_layers):
            v = torch.nn.functional.linear(z, next(it))
            z = z0 * lin(v) + z
        p = torch.sigmoid(lin(torch.relu(lin(z))))             # top 80-32-1
        assert next(it, None) is None
        return p

    for dense, idx, lab in _batches(dcfg, B, 3):
        ex.scatter_from_host(d, dense)
        for t, a in zip(s, idx):
            ex.scatter_from_host(t, a)
        ex.scatter_from_host(m.get_label_tensor(), lab)
        ex.train_step()
        loss = torch.nn.functional.binary_cross_entropy(replica(torch.tensor(dense), [torch.tensor(i) for i in idx]),
                                                        torch.tensor(lab))
        grads = torch.autograd.grad(loss, W)
        with torch.no_grad():
            for w, g, h in zip(W, grads, H):
                if optname == "sgd":
                    w -= lr * g
                else:          # tables: one accumulator per row (rows no lookup touched have g = 0 and stay)
                    h += (g * g).mean(1, keepdim=True) if id(w) in tables else g * g
                    w -= lr * g / (h.sqrt() + eps)
    for p, w, n in zip(m.parameters, W, names):
        np.testing.assert_allclose(p.get_weights(m), w.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=n)


def test_four_tables_run_as_one_embedding_group():
    from flexmi.core import LossType, MetricsType, SGDOptimizer
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    m = _cpu_model(16)
    build_dlrm(m, DLRMConfig.preset("tiny_dcn_multihot"))
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    embs = [op for op in m.layers if op.op_type == OperatorType.OP_EMBEDDING]
    assert [op.inputs[0].dims[1] for op in embs] == BAGS
    groups = {id(ex.group_of[op.guid]) for op in embs}
    assert len(groups) == 1 and ex.group_of[embs[0].guid] == embs
    names = [it.name for it in ex.prog_fwd]
    assert [n for n in names if n.startswith("embedding")] == ["embedding0.group_fwd"], names


# ------------------------------------------------------------------ HDF5 data
def _criteo_multihot(n, tables, bags, seed=0):
    rng = np.random.RandomState(seed)
    return {
        "X_int": np.log(rng.randint(0, 1000, (n, 13)).astype(np.float32) + 1),
        "X_cat": np.concatenate([rng.randint(0, r, (n, b)) for r, b in zip(tables, bags)], 1).astype(np.int64),
        "y": rng.randint(0, 2, n).astype(np.float32),
    }


def _tiny_model(dcfg, B):
    from flexmi.core import LossType, MetricsType, SGDOptimizer
    from flexmi.models.dlrm import build_dlrm
    m = _cpu_model(B)
    d, s, _ = build_dlrm(m, dcfg)
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    return m, m.init_layers(), d, s


def test_hdf5_feeds_each_table_its_columns(tmp_path, native):
    from flexmi.models.dlrm import DLRMConfig, HDF5DLRMData
    from flexmi.utils.hdf5 import write_h5
    dcfg = DLRMConfig.preset("tiny_dcn_multihot")
    arrays = _criteo_multihot(64, dcfg.embedding_size, BAGS)
    assert arrays["X_cat"].shape == (64, 14)
    path = str(tmp_path / "multihot.h5")
    write_h5(path, arrays)
    B = 16
    m, ex, d, s = _tiny_model(dcfg, B)
    data = HDF5DLRMData(m, d, s, dcfg, path)
    assert data.num_samples == 64 and data.nb == 4
    off = np.concatenate([[0], np.cumsum(BAGS)])
    for k in range(2):
        data.next_batch()
        for i, t in enumerate(s):
            got = np.asarray(ex.gather_to_host(t))
            assert got.shape == (B, BAGS[i])
            assert np.array_equal(got, arrays["X_cat"][k * B:(k + 1) * B, off[i]:off[i + 1]]), (k, i)
    data.close()
    # a width that is not the sum of the bag sizes is rejected, naming the width expected
    wide = dict(arrays, X_cat=np.concatenate([arrays["X_cat"], arrays["X_cat"][:, :2]], 1))
    assert wide["X_cat"].shape == (64, 16)
    bad = str(tmp_path / "wide.h5")
    write_h5(bad, wide)
    with pytest.raises(ValueError, match=r"X_cat must be integer \[N, 14\]"):
        HDF5DLRMData(m, d, s, dcfg, bad)


def test_hdf5_uniform_bag_file_stays_valid(tmp_path, native):
    from flexmi.models.dlrm import DLRMConfig, HDF5DLRMData
    from flexmi.utils.hdf5 import write_h5
    dcfg = DLRMConfig.parse_args(["dlrm", "--embedding-bag-size", "2"], DLRMConfig.preset("tiny_dcn"))
    arrays = _criteo_multihot(32, dcfg.embedding_size, [2] * 4)
    path = str(tmp_path / "uniform.h5")
    write_h5(path, arrays)
    m, ex, d, s = _tiny_model(dcfg, 16)
    data = HDF5DLRMData(m, d, s, dcfg, path)
    data.next_batch()
    for i, t in enumerate(s):
        assert np.array_equal(np.asarray(ex.gather_to_host(t)), arrays["X_cat"][:16, 2 * i:2 * i + 2])
    data.close()


def test_app_trains_the_multihot_preset_from_a_dataset(tmp_path, native):
    from flexmi.models.dlrm import DLRMConfig
    from flexmi.utils.hdf5 import write_h5
    spec = importlib.util.spec_from_file_location("dlrm_app", os.path.join(os.path.dirname(__file__), "..", "apps", "dlrm.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    path = str(tmp_path / "multihot.h5")
    write_h5(path, _criteo_multihot(64, DLRMConfig.preset("tiny_dcn_multihot").embedding_size, BAGS))
    sps, met = app.main(["--preset", "tiny_dcn_multihot", "--dataset", path, "-e", "1", "-b", "16", "--device", "cpu",
                         "--optimizer", "rowwise_adagrad", "--auc"])
    assert sps > 0 and met.train_all == 64
    assert np.isfinite(met.get_loss()) and np.isfinite(met.get_accuracy()) and 0.0 <= met.get_auc() <= 1.0
