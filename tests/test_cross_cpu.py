"""CrossCombine (the DCNv2 cross-layer combine ``y = x0 * t + x``), ``FFModel.cross_layer`` and the
DLRM ``dcn`` interaction on the fp32 CPU executor: the op against torch autograd, the fused model
against the same model composed from ``multiply`` + ``add``, the presets, and ``tiny_dcn`` trained
end to end against a torch replica."""
import itertools
import math

import numpy as np
import pytest
import torch


def _cpu_model(B, device="cpu"):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = device, "fp32", B
    return FFModel(cfg)


# ------------------------------------------------------------------ the op against autograd
SHAPE = (5, 24)
_CASES = [(three, accs, drop)
          for three in (False, True)
          for accs in itertools.product((False, True), repeat=3)
          for drop in ((), ("dx0",), ("dx",), ("dx0", "dx"))]


@pytest.mark.parametrize("three,accs,drop", _CASES)
def test_op_matches_autograd(three, accs, drop):
    from flexmi.ops.base import OpCtx
    m = _cpu_model(SHAPE[0])
    ins = [m.create_tensor(list(SHAPE)) for _ in range(3 if three else 2)]
    out = m.cross_combine(*ins)
    op = out.owner_op
    assert tuple(out.dims) == SHAPE and op.splittable_dims() == {0, 1} and not op.weights
    g = torch.Generator().manual_seed(11)
    vals = [torch.randn(SHAPE, generator=g, requires_grad=True) for _ in ins]
    dy = torch.randn(SHAPE, generator=g)
    ref = vals[0] * vals[1] + (vals[2] if three else vals[0])
    ref.backward(dy)

    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs = [v.detach().clone() for v in vals]
    ctx.outputs = [torch.full(SHAPE, float("nan"))]
    op.forward(ctx)
    assert not ctx.saved
    torch.testing.assert_close(ctx.outputs[0], ref.detach(), rtol=0, atol=1e-6)

    prev = [torch.randn(SHAPE, generator=g) for _ in ins]
    names = ["dx0", "dt", "dx"][:len(ins)]
    ctx.out_grads = [dy.clone()]
    ctx.in_grads = [None if n in drop else p.clone() for n, p in zip(names, prev)]
    ctx.in_grad_accumulate = list(accs[:len(ins)])
    op.backward(ctx)
    for n, got, p, acc, v in zip(names, ctx.in_grads, prev, ctx.in_grad_accumulate, vals):
        if n in drop:
            assert got is None
            continue
        want = v.grad + (p if acc else 0)
        torch.testing.assert_close(got, want, rtol=0, atol=1e-6, msg=lambda s, n=n: f"{n}: {s}")
    for a, v in zip(ctx.inputs, vals):                       # inputs untouched
        assert torch.equal(a, v.detach())
    assert torch.equal(ctx.out_grads[0], dy)


def test_same_tensor_twice_is_rejected():
    m = _cpu_model(4)
    z, t = m.create_tensor([4, 8]), m.create_tensor([4, 8])
    with pytest.raises(ValueError, match="two-input form"):
        m.cross_combine(z, t, z)
    with pytest.raises(ValueError, match="one shape"):
        m.cross_combine(z, t, m.create_tensor([4, 6]))
    n = len(m.layers)
    m.cross_combine(z, t)                                     # the accepted spelling
    assert len(m.layers) == n + 1 and len(m.layers[-1].inputs) == 2


# ------------------------------------------------------------------ fused against composed
def _cross_net(fused, B=16, D=24, r=8, nin=13, device="cpu"):
    """ReLU dense layer, three cross layers (fused, or composed from multiply + add), sigmoid dense layer."""
    from flexmi.core import ActiMode, LossType, MetricsType, SGDOptimizer
    m = _cpu_model(B, device)
    x = m.create_tensor([B, nin])
    z0 = z = m.dense(x, D, ActiMode.AC_MODE_RELU)
    for _ in range(3):
        if fused:
            z = m.cross_layer(z0, z, r)
        else:
            v = m.dense(z, r, ActiMode.AC_MODE_NONE, False)
            t = m.dense(v, D, ActiMode.AC_MODE_NONE, True)
            z = m.add(m.multiply(z0, t), z)
    m.dense(z, 1, ActiMode.AC_MODE_SIGMOID)
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    m.init_layers()
    return m, x


def fused_vs_composed(**kw):
    """Three SGD steps of the fused and the composed network from the same weights on the same data."""
    from flexmi.core.types import OperatorType
    mf, xf = _cross_net(True, **kw)
    mc, xc = _cross_net(False, **kw)
    B, nin = xf.dims
    combines = [op for op in mf.layers if op.op_type == OperatorType.OP_CROSS_COMBINE]
    assert [len(op.inputs) for op in combines] == [2, 3, 3]   # the first layer takes the two-input form
    assert not any(op.op_type == OperatorType.OP_CROSS_COMBINE for op in mc.layers)
    assert [tuple(p.dims) for p in mf.parameters] == [tuple(p.dims) for p in mc.parameters]
    start = [a.get_weights(mf).copy() for a in mf.parameters]
    for b, w0 in zip(mc.parameters, start):
        b.set_weights(mc, w0)
    rng = np.random.RandomState(5)
    for _ in range(3):
        xv = rng.randn(B, nin).astype(np.float32)
        lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
        for m, x in ((mf, xf), (mc, xc)):
            ex = m._ex()
            ex.scatter_from_host(x, xv)
            ex.scatter_from_host(m.get_label_tensor(), lab)
            ex.train_step()
    for a, b, w0 in zip(mf.parameters, mc.parameters, start):
        wa = a.get_weights(mf)
        np.testing.assert_allclose(wa, b.get_weights(mc), rtol=1e-5, atol=1e-6, err_msg=a.name)
        assert np.abs(wa - w0).max() > 1e-4, a.name          # every parameter, the cross layers' included, trained


def test_fused_equals_composed():
    fused_vs_composed(B=16, D=24, r=8)


def test_cross_layer_initialisers():
    from flexmi.core.types import OperatorType
    m = _cpu_model(4)
    x = m.create_tensor([4, 640])
    m.cross_layer(x, x, 384, name="c")
    v, u, c = m.layers
    assert (v.name, u.name, c.name) == ("c_v", "c_u", "c") and c.op_type == OperatorType.OP_CROSS_COMBINE
    assert [tuple(w.dims) for w in v.weights] == [(384, 640)]
    assert [tuple(w.dims) for w in u.weights] == [(640, 384), (640,)]
    m.compile()
    m.init_layers()
    std = math.sqrt(2.0 / (640 + 384))
    wv, wu, bu = v.weights[0].get_weights(m), u.weights[0].get_weights(m), u.weights[1].get_weights(m)
    # 245 760 samples each: the sample std of a normal is within 1 % of sigma far beyond 6 sigma
    assert abs(wv.std() / std - 1) < 0.01 and abs(wu.std() / std - 1) < 0.01
    assert abs(wv.mean()) < 0.01 * std * 6 and not np.array_equal(wv, wu.T)
    assert not bu.any()


# ------------------------------------------------------------------ presets and flags
def test_presets_and_flags():
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import MLPERF_TABLES, DLRMConfig, build_dlrm
    c = DLRMConfig.preset("mlperf_dcnv2")
    assert (c.arch_interaction_op, c.dcn_layers, c.dcn_rank, c.loss) == ("dcn", 3, 512, "bce")
    assert c.embedding_size == MLPERF_TABLES and c.sparse_feature_size == 128
    assert c.mlp_bot == [13, 512, 256, 128] and c.mlp_top[1:] == [1024, 1024, 512, 256, 1]
    t = DLRMConfig.preset("tiny_dcn")
    assert (t.arch_interaction_op, t.dcn_layers, t.dcn_rank, t.loss) == ("dcn", 2, 8, "bce")
    tiny = DLRMConfig.preset("tiny")
    assert (t.embedding_size, t.mlp_bot, t.mlp_top[1:]) == (tiny.embedding_size, tiny.mlp_bot, tiny.mlp_top[1:])
    assert (DLRMConfig().dcn_layers, DLRMConfig().dcn_rank) == (3, 512)
    for cfg, width, layers, rank in ((c, 27 * 128, 3, 512), (t, (1 + 4) * 16, 2, 8)):
        m = _cpu_model(8)
        build_dlrm(m, cfg)                                   # graph only: no table is allocated
        comb = [op for op in m.layers if op.op_type == OperatorType.OP_CROSS_COMBINE]
        assert len(comb) == layers and [len(op.inputs) for op in comb] == [2] + [3] * (layers - 1)
        assert all(tuple(op.outputs[0].dims) == (8, width) for op in comb)
        assert all(op.inputs[0] is comb[0].inputs[0] for op in comb)          # every layer multiplies by x_0
        k = m.layers.index(comb[-1])
        assert m.layers[k + 1].inputs[0] is comb[-1].outputs[0]              # the result feeds the top MLP
        assert tuple(m.layers[k + 1].weights[0].dims) == (cfg.mlp_top[1], width)
        assert tuple(m.layers[k - 2].weights[0].dims) == (rank, width)
    p = DLRMConfig.parse_args(["dlrm", "--arch-interaction-op", "dcn", "--arch-dcn-layers", "4", "--arch-dcn-rank", "32"])
    assert (p.arch_interaction_op, p.dcn_layers, p.dcn_rank) == ("dcn", 4, 32)
    p = DLRMConfig.parse_args(["dlrm", "--arch-dcn-rank", "16"], DLRMConfig.preset("tiny_dcn"))
    assert (p.dcn_layers, p.dcn_rank) == (2, 16)


def test_zoo_and_measure_know_the_op():
    from flexmi.core.types import OperatorType
    from flexmi.models.zoo import build
    from flexmi.runtime.measure import measure_op
    assert OperatorType.OP_CROSS_COMBINE == 104
    m = _cpu_model(16)
    build("dlrm-tiny_dcn", m)
    comb = [op for op in m.layers if op.op_type == OperatorType.OP_CROSS_COMBINE]
    assert len(comb) == 2
    for op in comb:                                          # both forms rebuild and time on the host
        f, b = measure_op(op, [(16, 80)] * len(op.inputs), [(16, 80)], reps=2, device="cpu")
        assert f > 0 and b > 0


# ------------------------------------------------------------------ tiny_dcn against a torch replica
def test_tiny_dcn_matches_torch_replica():
    from flexmi.core import LossType, MetricsType, SGDOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    B, lr = 16, 0.1
    dcfg = DLRMConfig.preset("tiny_dcn")
    m = _cpu_model(B)
    d, s, _ = build_dlrm(m, dcfg)
    m.compile(SGDOptimizer(m, lr), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    W = [torch.tensor(p.get_weights(m), dtype=torch.float32, requires_grad=True) for p in m.parameters]
    names = [p.name for p in m.parameters]

    def replica(dense, idx):
        it = iter(W)
        lin = lambda x: torch.nn.functional.linear(x, next(it), next(it))
        x = torch.relu(lin(torch.relu(lin(dense))))            # bottom 13-32-16
        embs = [next(it)[i[:, 0]] for i in idx]                # bag size 1
        z0 = z = torch.cat([x] + embs, 1)
        for _ in range(dcfg.dcn_layers):
            v = torch.nn.functional.linear(z, next(it))
            z = z0 * lin(v) + z
        p = torch.sigmoid(lin(torch.relu(lin(z))))             # top 80-32-1
        assert next(it, None) is None
        return p

    rng = np.random.RandomState(3)
    for _ in range(3):
        dense = rng.rand(B, 13).astype(np.float32)
        idx = [rng.randint(0, r, (B, 1)).astype(np.int64) for r in dcfg.embedding_size]
        lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
        ex.scatter_from_host(d, dense)
        for t, a in zip(s, idx):
            ex.scatter_from_host(t, a)
        ex.scatter_from_host(m.get_label_tensor(), lab)
        ex.train_step()
        loss = torch.nn.functional.binary_cross_entropy(replica(torch.tensor(dense), [torch.tensor(i) for i in idx]),
                                                        torch.tensor(lab))
        grads = torch.autograd.grad(loss, W)
        with torch.no_grad():
            for w, g in zip(W, grads):
                w -= lr * g
    for p, w, n in zip(m.parameters, W, names):
        np.testing.assert_allclose(p.get_weights(m), w.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
