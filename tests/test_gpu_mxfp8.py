"""csrc/kernels/mxfp8.hip: the quantisers bit for bit against flexmi.ops.mx.mx_quantize_torch, the block-scaled
GEMM against fp64 of the dequantised operands, and LinearMX on the GPU against the CPU backend."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}     # max-normalised, as tests/test_gpu_dot_wide.py
STEP_DIFF_MEASURED = 2.614e-3     # one step of _train, GPU vs CPU, largest of seeds 0..4 (profiles/mxfp8.txt)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def block_scaled(rows, cols, lo, hi, gen):
    e = torch.randint(lo, hi + 1, (rows, cols // 32), generator=gen).repeat_interleave(32, 1)
    return torch.ldexp(torch.randn(rows, cols, generator=gen), e)


def oracle_copies(x, fmt):
    from flexmi.ops.mx import mx_quantize_torch, pad128
    rc, rs, _ = mx_quantize_torch(x, 1, fmt)
    xp = torch.cat([x.float(), torch.zeros(pad128(x.shape[0]) - x.shape[0], x.shape[1])])
    cc, cs, _ = mx_quantize_torch(xp, 0, fmt)                            # the column-wise copy, before the transpose
    return rc.view(torch.uint8), rs, cc.view(torch.uint8).t().contiguous(), cs.t().contiguous()


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,C,ld", [(1, 32, 32), (33, 96, 96), (70, 160, 192)])
def test_quant_bit_equal(gpu, R, C, ld, dt, fmt):
    from flexmi.ops import _kernels as K
    g = torch.Generator().manual_seed(R + C)
    x = block_scaled(R, C, -20, 20, g)
    sat = torch.randn(32, generator=g) * 2.0 ** 2
    sat[5] = 1.9 * 2.0 ** 9                                            # the only large value: 1.9 * 2^emax after scaling
    sub = torch.randn(32, generator=g) * 8 * torch.where(torch.arange(32) % 2 == 0, 2.0 ** -9, 2.0 ** (-15 if fmt == "e4m3" else -30))
    sub[17] = -(2.0 ** 3)
    x[0, :32] = sat
    if C >= 96:
        x[R - 1, 32:64] = 0
        x[R // 2, 64:96] = sub
    x = x.to(dt)
    buf = torch.full((R, ld), 7.0, dtype=dt, device="cuda")
    buf[:, :C] = x.cuda()
    out = K.mx_alloc(R, C, "cuda")
    [t.fill_(0xAA) for t in out]
    K.mx_quant(buf[:, :C], int(fmt == "e5m2"), *out)
    for name, got, want in zip(("row codes", "row scales", "column codes", "column scales"), out, oracle_copies(x, fmt)):
        assert torch.equal(got.cpu(), want), name
    assert not out[2][:, R:].any(), "pad of the column-wise copy"


def mx_operand(rows, K, fmt, gen):
    from flexmi.ops.mx import mx_quantize_torch
    codes, scales, deq = mx_quantize_torch(block_scaled(rows, K, -8, 8, gen), 1, fmt)
    return codes.view(torch.uint8).cuda(), scales.cuda(), deq.double()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("fa", ["e4m3", "e5m2"])
@pytest.mark.parametrize("M,N,K,epi", [(1, 32, 32, "plain"), (16, 32, 128, "plain"), (130, 96, 160, "plain"),
                                       (257, 160, 416, "plain"), (130, 96, 160, "bias_relu"), (130, 96, 160, "acc")])
def test_gemm_against_fp64(gpu, M, N, K, epi, fa, dt):
    from flexmi.ops import _kernels as Kk
    g = torch.Generator().manual_seed(M + N + K)
    a, sa, a64 = mx_operand(M, K, fa, g)
    b, sb, b64 = mx_operand(N, K, "e4m3", g)
    ref = a64 @ b64.t()
    bias, out = None, torch.full((M, N), float("nan"), dtype=dt, device="cuda")
    if epi == "bias_relu":
        bias = (torch.randn(N, generator=g) * ref.abs().max().float()).cuda()
        ref = torch.relu(ref + bias.double().cpu())
    if epi == "acc":
        prev = (torch.randn(M, N, generator=g) * ref.abs().max().float()).to(dt)
        out.copy_(prev)
        ref = ref + prev.double()
    Kk.mx_gemm(a, sa, int(fa == "e5m2"), b, sb, 0, out, M, N, K, bias=bias, act=11 if epi == "bias_relu" else 10, beta=epi == "acc")
    assert rel_err(out, ref) < TOL[dt]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("act", [12, 11], ids=["sigmoid", "relu"])
def test_quant_dact(gpu, act, dt):
    from flexmi.ops import _kernels as K
    from flexmi.ops.linear import act_backward_torch
    R, C, g = 70, 96, torch.Generator().manual_seed(act)
    dy = block_scaled(R, C, -6, 6, g).to(dt).cuda()
    y = (torch.sigmoid if act == 12 else torch.relu)(torch.randn(R, C, generator=g)).to(dt).cuda()
    dpre = act_backward_torch(dy.float(), y.float(), act)                # fp32, by torch on the GPU
    db0 = torch.randn(C, generator=g).cuda()
    runs = []
    for _ in range(2):
        out, db = K.mx_alloc(R, C, "cuda"), db0.clone()
        K.mx_quant_dact(dy, y, act, *out, db)
        runs.append(out + (db,))
    for name, got, want in zip(("row codes", "row scales", "column codes", "column scales"), runs[0], oracle_copies(dpre.cpu(), "e5m2")):
        assert torch.equal(got.cpu(), want), name
    assert rel_err(runs[0][4], db0.double() + dpre.double().sum(0)) < 1e-4
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "two runs differ"


def _op_run(backend, dt, acc, tensors):
    from flexmi.core import FFConfig, FFModel
    from flexmi.core.types import ActiMode
    from flexmi.ops.base import OpCtx
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", 70
    m = FFModel(cfg)
    op = m.dense(m.create_tensor([70, 96]), 64, ActiMode.AC_MODE_RELU, fp8=True).owner_op
    dev = "cuda" if backend == "hip" else "cpu"
    x, w, b, dy, dx0, dw0, db0 = [t.to(dev) for t in tensors]
    ctx = OpCtx(op, 0, backend, dt)
    ctx.inputs, ctx.weights, ctx.wcompute = [x.to(dt)], [w, b], [w.to(dt)]
    ctx.outputs = [torch.empty(70, 64, dtype=dt, device=dev)]
    op.forward(ctx)
    ctx.out_grads, ctx.in_grads, ctx.in_grad_accumulate = [dy.to(dt)], [dx0.to(dt).clone()], [acc]
    ctx.weight_grads = [dw0.clone(), db0.clone()]
    op.backward(ctx)
    return ctx.outputs[0], ctx.in_grads[0], ctx.weight_grads[0], ctx.weight_grads[1]


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_op_gpu_matches_cpu(gpu, dt, acc):
    g = torch.Generator().manual_seed(2)
    tensors = [torch.randn(s, generator=g) for s in ((70, 96), (64, 96), (64,), (70, 64), (70, 96), (64, 96), (64,))]
    cpu, hip = _op_run("cpu", dt, acc, tensors), _op_run("hip", dt, acc, tensors)
    for name, c, h, tol in zip(("y", "dx", "dw", "db"), cpu, hip, (TOL[dt], TOL[dt], 1e-4, 1e-4)):
        assert rel_err(h, c) < tol, name


@functools.lru_cache(maxsize=None)
def _train(dev, graph=False, steps=3, seed=0):
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    from flexmi.core.types import ActiMode
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = 70, dev, "fp32", 5 + seed
    m = FFModel(cfg)
    x = m.create_tensor([70, 96])
    m.dense(m.dense(x, 64, ActiMode.AC_MODE_RELU, fp8=True), 32, fp8=True)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(seed)

    def feed():
        ex.scatter_from_host(x, rng.randn(70, 96).astype(np.float32))
        ex.scatter_from_host(m.get_label_tensor(), rng.randn(70, 32).astype(np.float32))

    run = ex.train_step
    for i in range(steps):
        feed()
        run()
        run = ex.capture_step() if graph and i == 0 else run
    if dev == "gpu":
        torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters]


def test_model_graph_equals_eager(gpu):
    for a, b in zip(_train("gpu", False), _train("gpu", True)):
        assert np.array_equal(a, b)


def test_model_step_gpu_vs_cpu(gpu):
    worst = max(np.abs(a - b).max() / np.abs(a).max() for a, b in zip(_train("cpu", steps=1), _train("gpu", steps=1)))
    assert worst < 4 * STEP_DIFF_MEASURED
