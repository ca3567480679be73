"""DCNv2 cross layers on MI355X: the ``cross.hip`` kernels against a float64 oracle (both storage
types, both forms, every accumulate combination, vector / tail / scalar / second-sweep sizes), the
Linear kernels at the cross layers' GEMM shapes, and ``tiny_dcn`` GPU against CPU, captured against
eager, fused against composed."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (elements, view offset in elements from a 16-B aligned base)
#   39      = 4 vectors of 8 + a 7-element tail
#   120     = 5 x 24, vectors only
#   120 + 1 = the same on a base offset by one element: no operand is 16-B aligned, scalar path
#   1300 x 3456 > 2048 blocks x 256 lanes x 8 elements = 4 194 304: a second grid-stride sweep
SIZES = {"39": (39, 0), "5x24": (120, 0), "5x24+1": (120, 1), "1300x3456": (1300 * 3456, 0)}
GUARD = 8            # sentinel elements on either side of every buffer (8 x 2 B keeps 16-B alignment)


class Buf:
    """n elements of ``dtype`` inside a sentinel-filled allocation, ``off`` elements past alignment."""

    def __init__(self, n, dtype, off, gen, dev):
        self.whole = torch.full((n + 2 * GUARD + off,), 777.0, dtype=dtype, device=dev)
        self.t = self.whole[GUARD + off: GUARD + off + n]
        self.t.copy_(torch.randn(n, generator=gen, device=dev).to(dtype))   # exact values of the storage type
        self.before = self.whole.clone()
        assert (self.t.data_ptr() % 16 == 0) == (off == 0) and self.t.is_contiguous()

    def f64(self):
        return self.before[self.t.storage_offset(): self.t.storage_offset() + self.t.numel()].double()

    def guards_intact(self):
        lo, hi = self.t.storage_offset(), self.t.storage_offset() + self.t.numel()
        return torch.equal(self.whole[:lo], self.before[:lo]) and torch.equal(self.whole[hi:], self.before[hi:])

    def untouched(self):
        return torch.equal(self.whole, self.before)


def _bound(dtype):
    # S = sum of |terms| of a result.  fp32: at most three roundings (product, sums; fewer when fused) of
    # partial results no larger than S, allowed 4 x 2^-24 S.  bf16: fp32 arithmetic, then ONE rounding
    # to 8 significant bits on store (2^-9 S) -- allowed 2 x 2^-9 S.
    return 4 * 2.0 ** -24 if dtype == torch.float32 else 2 * 2.0 ** -9


def _check(got, terms, dtype, what):
    ref = sum(terms)
    S = sum(t.abs() for t in terms)
    err = (got.t.double() - ref).abs()
    bad = err > _bound(dtype) * S
    assert not bad.any(), (what, int(bad.sum()), float((err / S.clamp_min(1e-300)).max()))
    assert got.guards_intact(), what + ": wrote outside its buffer"


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cross_kernels_vs_float64(gpu, dtype, size):
    from flexmi.ops import _kernels as Kk
    n, off = SIZES[size]
    gen = torch.Generator(device=gpu).manual_seed(n + off)
    mk = lambda: Buf(n, dtype, off, gen, gpu)
    x0, t, x, dy = mk(), mk(), mk(), mk()
    inputs = (x0, t, x, dy)
    a, b, c, g = (v.f64() for v in inputs)
    for three in (True, False):
        y = mk()
        Kk.cross_forward(x0.t, t.t, x.t if three else None, y.t)
        _check(y, [a * b, c if three else a], dtype, f"fwd three={three}")
        combos = [(accs, ()) for accs in itertools.product((False, True), repeat=3)]
        combos += [((True, False, True), ("dx0",)), ((False, True, False), ("dx",)), ((True, True, True), ("dx0", "dx"))]
        for (acct, acc0, accx), drop in combos:
            if not three:
                drop = tuple(set(drop) | {"dx"})              # the two-input form has no dx
            dt, d0, dx = mk(), mk(), mk()
            pt, p0, px = dt.f64(), d0.f64(), dx.f64()
            Kk.cross_backward(dy.t, x0.t, t.t, dt.t, None if "dx0" in drop else d0.t, None if "dx" in drop else dx.t,
                              acct, acc0, accx, not three)
            what = f"bwd three={three} acc={(acct, acc0, accx)} drop={drop}"
            _check(dt, [g * a] + ([pt] if acct else []), dtype, what + " dt")
            if "dx0" in drop:
                assert d0.untouched(), what
            else:
                _check(d0, [g * b] + ([] if three else [g]) + ([p0] if acc0 else []), dtype, what + " dx0")
            if "dx" in drop:
                assert dx.untouched(), what
            else:
                _check(dx, [g] + ([px] if accx else []), dtype, what + " dx")
    dt = mk()                                                  # dt absent too: only dx0 and dx are produced
    d0, dx = mk(), mk()
    Kk.cross_backward(dy.t, x0.t, t.t, None, d0.t, dx.t, False, False, False, False)
    _check(d0, [g * b], dtype, "no dt: dx0")
    _check(dx, [g], dtype, "no dt: dx")
    assert dt.untouched()
    for v in inputs:                                           # x0, t, x, dy bit-identical afterwards
        assert v.untouched()


def test_cross_kernels_reject_mismatched_operands(gpu):
    from flexmi.ops import _kernels as Kk
    a = torch.zeros(5, 24, device=gpu)
    with pytest.raises(RuntimeError, match="cross_fwd"):
        Kk.cross_forward(a, torch.zeros(5, 23, device=gpu), None, a.clone())
    with pytest.raises(RuntimeError, match="cross_fwd"):
        Kk.cross_forward(a, a.clone().bfloat16(), None, a.clone())
    with pytest.raises(RuntimeError, match="cross_bwd"):
        Kk.cross_backward(a, a.clone(), a.clone(), a.clone(), torch.zeros(5, 48, device=gpu)[:, ::2], None, 0, 0, 0, True)
    with pytest.raises(RuntimeError, match="no dx"):
        Kk.cross_backward(a, a.clone(), a.clone(), a.clone(), a.clone(), a.clone(), 0, 0, 0, True)


# ------------------------------------------------------------------ the cross layers' GEMM shapes
def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.mark.parametrize("M,K,N", [(256, 3456, 512), (256, 512, 3456)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_linear_at_cross_shapes(gpu, dtype, M, K, N):
    """V (3456 -> 512, no bias) and U (512 -> 3456, bias) of the MLPerf DCNv2 layer, no activation.  fp32 at
    the 1e-4 of test_gpu_fp32 / test_gpu_fp32_split; bf16 at test_gpu_kernels' GEMM bounds: 1e-2 into a bf16
    result, 2e-3 into an fp32 one (the weight and bias gradients)."""
    from flexmi.ops import _kernels as Kk
    torch.manual_seed(M + K + N)
    bias = N == 3456
    x = torch.randn(M, K, device=gpu).to(dtype)
    w = (torch.randn(N, K, device=gpu) / K ** 0.5).to(dtype)
    b = torch.randn(N, device=gpu) if bias else None
    y = torch.empty(M, N, device=gpu, dtype=dtype)
    Kk.linear_forward(x, w, b, 10, y)
    ref = x.double() @ w.double().t() + (b.double() if bias else 0)
    out_tol = 1e-4 if dtype == torch.float32 else 1e-2
    acc_tol = 1e-4 if dtype == torch.float32 else 2e-3
    assert rel_err(y, ref) < out_tol
    dy = torch.randn(M, N, device=gpu).to(dtype)
    dx = torch.randn(M, K, device=gpu).to(dtype)
    dx0 = dx.double().clone()
    dw = torch.randn(N, K, device=gpu)
    dw0 = dw.double().clone()
    db = torch.randn(N, device=gpu) if bias else None
    db0 = db.double().clone() if bias else None
    Kk.linear_backward(x, w, y, dy, 10, dx, True, dw, db, {})
    assert rel_err(dx, dx0 + dy.double() @ w.double()) < out_tol
    assert rel_err(dw.double() - dw0, dy.double().t() @ x.double()) < acc_tol
    if bias:
        assert rel_err(db.double() - db0, dy.double().sum(0)) < acc_tol


# ------------------------------------------------------------------ tiny_dcn end to end
def test_tiny_dcn_gpu_matches_cpu(gpu):
    from flexmi.core import FFConfig, FFModel, SGDOptimizer, LossType, MetricsType
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    B = 128
    rng = np.random.RandomState(1)
    dcfg = DLRMConfig.preset("tiny_dcn")
    dense = rng.rand(B, 13).astype(np.float32)
    sp = [rng.randint(0, r, (B, 1)).astype(np.int64) for r in dcfg.embedding_size]
    lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
    out = {}
    for dev in ("cpu", "gpu"):
        cfg = FFConfig()
        cfg.batchSize = B
        cfg.device = dev
        cfg.compute_dtype = "bf16" if dev == "gpu" else "fp32"
        m = FFModel(cfg)
        d, s, p = build_dlrm(m, dcfg)
        assert sum(op.op_type == OperatorType.OP_CROSS_COMBINE for op in m.layers) == 2
        m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
        ex = m.init_layers()
        for _ in range(4):
            dd = np.zeros((B, d.dims[1]), np.float32)
            dd[:, :13] = dense
            ex.scatter_from_host(d, dd)
            for t, a in zip(s, sp):
                ex.scatter_from_host(t, a)
            ex.scatter_from_host(m.get_label_tensor(), lab)
            ex.train_step()
        ws = [w.get_weights(m) for w in m.parameters]
        ws[0] = ws[0][:, :13]   # drop the (unused, zero-input) padding columns of the first layer
        out[dev] = (ws, m.get_perf_metrics().get_loss())
    assert len(out["cpu"][0]) == len(out["gpu"][0]) == 18
    for a, b in zip(out["cpu"][0], out["gpu"][0]):
        assert np.abs(a - b).max() < 3e-2 * max(1.0, np.abs(a).max()), (a.shape,)
    assert abs(out["cpu"][1] - out["gpu"][1]) < 2e-2


def test_tiny_dcn_hip_graph_capture_matches_eager(gpu):
    from flexmi.core import FFConfig, FFModel, SGDOptimizer, LossType, MetricsType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm, SyntheticDLRMData
    res = []
    for use_graph in (False, True):
        cfg = FFConfig()
        cfg.batchSize = 512
        cfg.seed = 3
        m = FFModel(cfg)
        dcfg = DLRMConfig.preset("tiny_dcn")
        d, s, p = build_dlrm(m, dcfg)
        m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
        ex = m.init_layers()
        data = SyntheticDLRMData(m, d, s, dcfg, num_batches=1)
        data.next_batch()
        if use_graph:
            ex.train_step()
            run = ex.capture_step()
            for _ in range(3):
                run()
        else:
            for _ in range(4):
                ex.train_step()
        torch.cuda.synchronize()
        res.append([w.get_weights(m) for w in m.parameters])
    for a, b in zip(*res):
        assert np.allclose(a, b, atol=1e-5), a.shape


def test_fused_equals_composed_fp32(gpu):
    """Same weights, same GEMMs; only the element-wise pass differs (one fused pass against multiply + add)."""
    from tests.test_cross_cpu import fused_vs_composed
    fused_vs_composed(B=128, D=80, r=8, nin=16, device="gpu")
