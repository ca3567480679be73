"""Dot interaction with 33..64 features (csrc/kernels/interaction_wide.hip): the wide kernels vs a
float64 oracle in bf16 and fp32, on strided operands, with the fused activation backward, and a
40-table DLRM through build_dlrm on the GPU (eager and as a captured hipGraph step) vs the CPU."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# max-normalised bounds of the existing interaction tests: set by the output rounding (fp32
# accumulation), so they do not depend on F
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}
BWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _pairs(F, selfi):
    return zip(*[(i, j) for i in range(F) for j in range(i + (1 if selfi else 0))])


def _oracle(zs, dy, D, W, selfi, act0=False):
    """float64 forward row [x | pairs | 0] and input gradients of the given (storage-precision) operands."""
    F = len(zs)
    Z = torch.stack([z.double() for z in zs], 1)
    li, lj = _pairs(F, selfi)
    ref = torch.zeros(Z.shape[0], W, dtype=torch.float64, device=Z.device)
    ref[:, :D] = Z[:, 0]
    ref[:, D:D + len(li)] = (Z @ Z.transpose(1, 2))[:, li, lj]
    dG = torch.zeros(Z.shape[0], F, F, dtype=torch.float64, device=Z.device)
    dG[:, li, lj] = dy[:, D:D + len(li)].double()
    dZ = (dG + dG.transpose(1, 2)) @ Z
    dZ[:, 0] += dy[:, :D].double()
    if act0:
        dZ[:, 0] *= (Z[:, 0] > 0).double()
    return ref, dZ


def _check(zs, y, dy, dz, D, selfi, dt, act0=False):
    """Forward into the 7-prefilled `y`, backward into `dz` (accumulating into every odd input; a
    None entry is an input without a gradient), both against the oracle."""
    from flexmi.ops import _kernels as Kk
    F, W = len(zs), y.shape[1]
    ref, dZ = _oracle(zs, dy, D, W, selfi, act0)
    Kk.dot_interaction_forward(zs, y, selfi)
    assert rel_err(y, ref) < FWD_TOL[dt]
    assert (y[:, D + F * (F + (1 if selfi else -1)) // 2:] == 0).all()
    old = [None if g is None else g.double().clone() for g in dz]
    accs = [i % 2 == 1 for i in range(F)]
    Kk.dot_interaction_backward(zs, dy, dz, accs, selfi, act0=11 if act0 else 10)
    for i in range(F):
        if dz[i] is not None:
            assert rel_err(dz[i], dZ[:, i] + (old[i] if accs[i] else 0)) < BWD_TOL[dt], i


def _width(F, D, selfi):
    return (D + F * (F + (1 if selfi else -1)) // 2 + 15) // 16 * 16


def _cases():
    from flexmi.ops import _kernels as Kk
    big = 4 * Kk.C().dot_block_cap() + 3   # a second, prefetched sample per wave and a ragged last round
    return [(33, 32, False, 300), (64, 128, False, 300), (48, 64, True, 300), (40, 16, False, 300),
            (64, 128, False, big)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", range(5))
def test_dot_wide_vs_float64(gpu, case, dt):
    F, D, selfi, B = _cases()[case]
    torch.manual_seed(9)
    zs = [torch.randn(B, D, device=gpu).to(dt) for _ in range(F)]
    W = _width(F, D, selfi)
    dz = [torch.randn(B, D, device=gpu).to(dt) for _ in range(F)]
    dz[32] = None
    _check(zs, torch.full((B, W), 7.0, device=gpu, dtype=dt), torch.randn(B, W, device=gpu).to(dt), dz, D, selfi, dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dot_wide_strided(gpu, dt):
    """Inputs and gradients as column slices of one [B, F*D] buffer each, the output and dOut as the
    leading columns of wider buffers."""
    F, D, B = 40, 64, 300
    torch.manual_seed(11)
    W = _width(F, D, False)
    zbuf = torch.randn(B, F * D, device=gpu).to(dt)
    gbuf = torch.randn(B, F * D, device=gpu).to(dt)
    zs = [zbuf[:, i * D:(i + 1) * D] for i in range(F)]
    dz = [gbuf[:, i * D:(i + 1) * D] for i in range(F)]
    dz[32] = None
    ybuf = torch.full((B, W + 48), 7.0, device=gpu, dtype=dt)
    dybuf = torch.randn(B, W + 32, device=gpu).to(dt)
    _check(zs, ybuf[:, :W], dybuf[:, :W], dz, D, False, dt)
    assert (ybuf[:, W:] == 7).all()


def test_dot_wide_f32_act0(gpu):
    F, D, B = 40, 64, 300
    torch.manual_seed(10)
    zs = [torch.randn(B, D, device=gpu) for _ in range(F)]
    zs[0] = torch.relu(zs[0])
    W = _width(F, D, False)
    dz = [torch.randn(B, D, device=gpu) for _ in range(F)]
    _check(zs, torch.full((B, W), 7.0, device=gpu), torch.randn(B, W, device=gpu), dz, D, False, torch.float32, act0=True)


def test_dot_wide_f32_split_forward_binades(gpu):
    """The fp32 forward runs on the bf16 matrix cores through the exact three-way split: operands
    spanning 24 binades, per-element error against the magnitude of the product sums (|Z||Z|^T)."""
    from flexmi.ops import _kernels as Kk
    F, D, B = 64, 128, 300
    torch.manual_seed(19)
    zs = [torch.randn(B, D, device=gpu) * torch.exp2(torch.randint(-12, 12, (B, D), device=gpu).float())
          for _ in range(F)]
    W = _width(F, D, False)
    y = torch.full((B, W), 7.0, device=gpu)
    Kk.dot_interaction_forward(zs, y, False)
    ref, _ = _oracle(zs, torch.zeros(B, W, device=gpu), D, W, False)
    za = [z.abs() for z in zs]
    scale, _ = _oracle(za, torch.zeros(B, W, device=gpu), D, W, False)
    n = D + F * (F - 1) // 2
    err = ((y.double() - ref).abs() / scale.clamp_min(1e-30))[:, :n].max().item()
    assert err < 1e-5, err


@functools.lru_cache(maxsize=None)
def _dlrm40(dev, graph=False, B=256, steps=3):
    """3 SGD steps of a 40-table fp32 DLRM (F = 41, D = 32) built with build_dlrm."""
    from flexmi.core import FFConfig, FFModel, SGDOptimizer, LossType, MetricsType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    rows = [3, 7, 16, 40, 64, 2000, 5000, 3000] * 5
    dcfg = DLRMConfig(32, rows, [13, 64, 32], [0, 64, 1], 1, -1, -1, 0.0, "dot", "", -1, "bce", "wide40")
    rng = np.random.RandomState(0)
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = B, dev, "fp32", 5
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, dcfg)
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()

    def feed():
        dd = np.zeros((B, d.dims[1]), np.float32)
        dd[:, :13] = rng.rand(B, 13)
        ex.scatter_from_host(d, dd)
        for t, r in zip(s, rows):
            ex.scatter_from_host(t, rng.randint(0, r, (B, 1)).astype(np.int64))
        ex.scatter_from_host(m.get_label_tensor(), rng.randint(0, 2, (B, 1)).astype(np.float32))

    feed()
    ex.train_step()
    run = ex.capture_step() if graph else ex.train_step
    for _ in range(1, steps):
        feed()
        run()
    if dev == "gpu":
        torch.cuda.synchronize()
    ws = [w.get_weights(m) for w in m.parameters]
    ws[0] = ws[0][:, :13]   # the GPU pads the 13 dense features with zero input columns
    return ws, m.get_perf_metrics().get_loss()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_dlrm_40_tables_gpu_matches_cpu(gpu, graph):
    cpu, g = _dlrm40("cpu"), _dlrm40("gpu", graph)
    for a, b in zip(cpu[0], g[0]):
        assert np.abs(a - b).max() / max(np.abs(a).max(), 1e-6) < 1e-4, a.shape
    assert abs(cpu[1] - g[1]) < 1e-4 * max(1.0, abs(cpu[1]))
