"""csrc/kernels/glu.hip: the fused SwiGLU / GeGLU forward and the element-wise kernels against fp64, GatedLinear on the
GPU against the CPU backend in both forward forms, and one training step of a Llama-style encoder layer."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}     # max-normalised, as tests/test_gpu_mxfp8.py
STEP_DIFF_MEASURED = 6.130e-3     # one step of _train, bf16 GPU vs fp32 CPU, largest of seeds 0..4 (profiles/glu.txt)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def act64(g, act, grad=False):
    """fp64 act(g), or act'(g) by autograd"""
    g = g.double().clone().requires_grad_(grad)
    a = F.silu(g) if act == "silu" else F.gelu(g)
    return torch.autograd.grad(a.sum(), g)[0] if grad else a


def _op(act, M, H, FF):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", M
    m = FFModel(cfg)
    return m.gated_dense(m.create_tensor([M, H]), FF, act).owner_op


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("M,FF,H,sliced", [(1, 4, 8, False), (128, 64, 64, False), (256, 128, 192, False),
                                          (130, 72, 136, False), (130, 72, 136, True)])
def test_fused_forward_against_fp64(gpu, monkeypatch, M, FF, H, sliced, act):
    from flexmi.ops import gated
    from flexmi.ops.base import OpCtx
    monkeypatch.setattr(gated, "FORM", "fused")
    g = torch.Generator().manual_seed(M + FF + H)
    x = (torch.randn(M, H, generator=g) * (2 / H ** 0.5)).bfloat16()          # g ~ N(0, 2^2): both tails of the gates
    w = (torch.randn(2 * FF, H, generator=g) * torch.tensor([1.0, 0.5]).repeat_interleave(FF)[:, None]).bfloat16()
    xbuf = torch.zeros(M, H + (24 if sliced else 0), dtype=torch.bfloat16, device="cuda")
    hbuf = torch.full((M, FF + (16 if sliced else 0)), float("nan"), dtype=torch.bfloat16, device="cuda")
    xs, hs = (xbuf[:, 8:8 + H], hbuf[:, 8:8 + FF]) if sliced else (xbuf, hbuf)
    xs.copy_(x)
    ctx = OpCtx(_op(act, M, H, FF), 0, "hip", torch.bfloat16)
    ctx.inputs, ctx.wcompute, ctx.outputs = [xs], [w.cuda()], [hs]
    ctx.saved["gu"] = torch.full((M, 2 * FF), float("nan"), dtype=torch.bfloat16, device="cuda")
    ctx.op.forward(ctx)
    gu = ctx.saved["gu"].double().cpu()
    assert rel_err(gu, x.double() @ w.double().t()) < 1e-2, "gu"
    assert rel_err(hs, act64(gu[:, :FF], act) * gu[:, FF:]) < 1e-2, "h"
    assert not sliced or torch.isnan(torch.cat([hbuf[:, :8], hbuf[:, 8 + FF:]], 1)).all(), "the padding of h was written"


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,FF", [(3, 4), (33, 20), (70, 264)])
def test_act_kernels_against_fp64(gpu, M, FF, dt, act):
    from flexmi.ops import _kernels as K
    from flexmi.ops.gated import ACTIVATIONS
    g = torch.Generator().manual_seed(M + FF)
    gu = torch.randn(M, 2 * FF, generator=g) * 2
    gu[0, :4] = torch.tensor([-1.2785, -1.2780, -0.7520, -0.7515])           # either side of the roots of silu' and gelu'
    gu, dh = gu.to(dt).cuda(), torch.randn(M, FF, generator=g).to(dt).cuda()
    h = torch.full((M, FF), float("nan"), dtype=dt, device="cuda")
    dgu = torch.full((M, 2 * FF), float("nan"), dtype=dt, device="cuda")
    K.glu_act_fwd(gu, h, ACTIVATIONS[act])
    K.glu_act_bwd(dh, gu, dgu, ACTIVATIONS[act])
    g64, u64, dh64 = gu[:, :FF].double().cpu(), gu[:, FF:].double().cpu(), dh.double().cpu()
    assert rel_err(h, act64(g64, act) * u64) < TOL[dt]
    assert rel_err(dgu[:, :FF], dh64 * u64 * act64(g64, act, grad=True)) < TOL[dt], "dg"
    assert rel_err(dgu[:, FF:], dh64 * act64(g64, act)) < TOL[dt], "du"


def _two_ops(backend, dt, acc, tensors, B=3, T=43, H=72, FF=136, O=24):
    """gated_dense -> dense: one forward and backward of both ops on their OpCtx"""
    from flexmi.core import FFConfig, FFModel
    from flexmi.ops.base import OpCtx
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", B
    m = FFModel(cfg)
    top = m.dense(m.gated_dense(m.create_tensor([B, T, H]), FF, "silu"), O).owner_op
    glu = top.inputs[0].owner_op
    dev = "cuda" if backend == "hip" else "cpu"
    x, wk, wd, bd, dy, dx0 = [t.to(dev) for t in tensors]
    new = lambda *s, d=dt: torch.zeros(s, dtype=d, device=dev)     # noqa: E731
    c1, c2 = OpCtx(glu, 0, backend, dt), OpCtx(top, 0, backend, dt)
    c1.inputs, c1.weights, c1.wcompute, c1.outputs = [x.to(dt)], [wk], [wk.to(dt)], [new(B, T, FF)]
    c2.inputs, c2.weights, c2.wcompute, c2.outputs = c1.outputs, [wd, bd], [wd.to(dt)], [new(B, T, O)]
    glu.forward(c1)
    top.forward(c2)
    c2.out_grads, c2.in_grads, c2.in_grad_accumulate = [dy.to(dt)], [new(B, T, FF)], [False]
    c2.weight_grads = [new(O, FF, d=torch.float32), new(O, d=torch.float32)]
    top.backward(c2)
    c1.out_grads, c1.in_grads, c1.in_grad_accumulate = c2.in_grads, [dx0.to(dt).clone()], [acc]
    c1.weight_grads = [new(2 * FF, H, d=torch.float32)]
    glu.backward(c1)
    return c2.outputs[0], c1.in_grads[0], c1.weight_grads[0]


@pytest.mark.parametrize("dt,form,acc", [(torch.float32, "auto", False), (torch.bfloat16, "fused", True),
                                         (torch.bfloat16, "composed", False)], ids=["fp32", "bf16-fused", "bf16-composed"])
def test_op_gpu_matches_cpu(gpu, monkeypatch, dt, form, acc):
    from flexmi.ops import gated
    monkeypatch.setattr(gated, "FORM", form)
    g = torch.Generator().manual_seed(2)
    B, T, H, FF, O = 3, 43, 72, 136, 24
    shapes = ((B, T, H), (2 * FF, H), (O, FF), (O,), (B, T, O), (B, T, H))
    tensors = [torch.randn(s, generator=g) * k for s, k in zip(shapes, (1, H ** -0.5, FF ** -0.5, 1, 1, 1))]
    cpu, hip = _two_ops("cpu", dt, acc, tensors), _two_ops("hip", dt, acc, tensors)
    for name, c, h in zip(("y", "dx", "dw"), cpu, hip):
        assert rel_err(h, c) < TOL[dt], name


@functools.lru_cache(maxsize=None)
def _train(dev, seed=0):
    """one SGD step of a Llama-style layer (RMSNorm, rotary grouped-query attention, SwiGLU, no bias): bf16 on the GPU,
    where "auto" takes the fused forward, against the fp32 CPU backend.  The layer's output is the model's: a head with
    a zero-initialised bias would be compared relative to lr * its gradient, a sum that cancels (0.31 at seed 2)"""
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    B, T, E = 4, 40, 64
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = B, dev, "bf16" if dev == "gpu" else "fp32", 5 + seed
    m = FFModel(cfg)
    x = m.create_tensor([B, T, E])
    m.transformer_encoder_layer(x, 2, 136, causal=True, norm_first=True, name="l", attention_bias=False, num_kv_heads=1,
                                rope_base=10000.0, ffn="swiglu", rms_norm=True, ffn_bias=False)
    m.compile(SGDOptimizer(m, 0.01), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(seed)
    ex.scatter_from_host(x, rng.randn(B, T, E).astype(np.float32))
    ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, T, E).astype(np.float32))
    ex.train_step()
    if dev == "gpu":
        torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters]


def step_diff(seed):
    return max(np.abs(a - b).max() / np.abs(a).max() for a, b in zip(_train("cpu", seed), _train("gpu", seed)))


def test_llama_step_gpu_vs_cpu(gpu):
    assert step_diff(0) < 4 * STEP_DIFF_MEASURED
