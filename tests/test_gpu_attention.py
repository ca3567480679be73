"""Fused attention (csrc/kernels/attention.hip): the kernels against a float64 oracle in bf16 and
fp32 at the smallest shapes that reach every tile edge, the online rescale, strided operands with
accumulate flags and an absent gradient, run-to-run determinism, and a two-block self-attention model
on the GPU (eager and as a captured hipGraph step) against the CPU backend."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the max-normalised bounds of tests/test_gpu_dot_wide.py: fp32 accumulation, one storage rounding
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}
BWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _oracle(q, k, v, dout, heads, causal):
    """float64 output and input gradients of the given (storage-precision) operands."""
    B, Tq, E = q.shape
    ins = [t.double().clone().requires_grad_() for t in (q, k, v)]
    sp = lambda t: t.reshape(B, t.shape[1], heads, E // heads).transpose(1, 2)   # noqa: E731
    s = sp(ins[0]) @ sp(ins[1]).transpose(-1, -2) * (E // heads) ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(Tq, k.shape[1], dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    out = (torch.softmax(s, -1) @ sp(ins[2])).transpose(1, 2).reshape(B, Tq, E)
    out.backward(dout.double())
    return out.detach(), [t.grad for t in ins]


def _check(q, k, v, out, dout, grads, accs, heads, causal, dt):
    """Forward into `out`, backward into `grads` (a None entry is an absent gradient), both against the oracle."""
    from flexmi.ops import _kernels as Kk
    ref, dref = _oracle(q, k, v, dout, heads, causal)
    lse = torch.empty(q.shape[0], heads, q.shape[1], device=q.device)
    scale = (q.shape[2] // heads) ** -0.5
    Kk.attention_forward(q, k, v, out, lse, heads, causal, scale)
    err = [rel_err(out, ref)]
    old = [None if g is None else g.double().clone() for g in grads]
    Kk.attention_backward(q, k, v, out, dout, lse, *grads, accs, heads, causal, scale)
    err += [rel_err(g, d + (o if a else 0)) for g, d, o, a in zip(grads, dref, old, accs) if g is not None]
    print("rel_err out, grads:", err)
    assert err[0] < FWD_TOL[dt] and max(err[1:]) < BWD_TOL[dt], err


# (B, heads, dh, Tq, Tk, causal, rescale, accumulate flags), each the smallest shape at which one
# mechanism can break.  With one key dq and dk are exactly zero and a zero reference has no scale to
# normalise by, so that case checks both on top of an earlier value.
CASES = [(2, 1, 32, 1, 1, False, False, (True, True, False)), (3, 2, 64, 64, 64, True, False, (False, True, False)),
         (1, 2, 128, 130, 130, True, False, (True, False, True)), (2, 3, 64, 33, 70, False, False, (False, True, False)),
         (2, 2, 32, 200, 17, False, False, (False, False, True)), (1, 1, 64, 40, 200, False, True, (False, True, False))]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(x)) for x in c[:7]))
def test_attention_vs_float64(gpu, case, dt):
    B, H, dh, Tq, Tk, causal, rescale, accs = case
    torch.manual_seed(7)
    q, k, v = (torch.randn(B, T, H * dh, device=gpu) for T in (Tq, Tk, Tk))
    if rescale:
        q, k = q * 8, k * (1 + torch.arange(Tk, device=gpu) / 50.0)[None, :, None]
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    grads = [torch.randn_like(t) for t in (q, k, v)]
    _check(q, k, v, torch.full_like(q, 7.0), torch.randn(B, Tq, H * dh, device=gpu).to(dt), grads, accs, H, causal, dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attention_strided(gpu, dt):
    """q/k/v and their gradients as column slices of [B, T, 3E] buffers, out and dOut as the leading
    columns of wider ones; then the same with dk absent."""
    B, H, dh, T = 2, 2, 32, 70
    E = H * dh
    torch.manual_seed(8)
    qkv = torch.randn(B, T, 3 * E, device=gpu).to(dt)
    obuf = torch.full((B, T, E + 16), 7.0, device=gpu, dtype=dt)
    dobuf = torch.full((B, T, E + 32), 7.0, device=gpu, dtype=dt)
    dobuf[:, :, :E] = torch.randn(B, T, E, device=gpu).to(dt)
    for absent in (None, 1):
        gbuf = torch.randn(B, T, 3 * E, device=gpu).to(dt)
        grads = [None if i == absent else gbuf[:, :, i * E:(i + 1) * E] for i in range(3)]
        keep = gbuf[:, :, E:2 * E].clone()
        _check(*(qkv[:, :, i * E:(i + 1) * E] for i in range(3)), obuf[:, :, :E], dobuf[:, :, :E], grads,
               (True, False, True), H, True, dt)
        assert (obuf[:, :, E:] == 7).all() and (dobuf[:, :, E:] == 7).all()
        assert absent is None or torch.equal(gbuf[:, :, E:2 * E], keep)


def test_attention_backward_is_deterministic(gpu):
    from flexmi.ops import _kernels as Kk
    B, H, dh, Tq, Tk = 2, 3, 64, 133, 270
    torch.manual_seed(9)
    q, k, v = (torch.randn(B, T, H * dh, device=gpu).bfloat16() for T in (Tq, Tk, Tk))
    out, dout = torch.empty_like(q), torch.randn_like(q)
    lse = torch.empty(B, H, Tq, device=gpu)
    Kk.attention_forward(q, k, v, out, lse, H, False, 0.125)
    runs = []
    for _ in range(2):
        g = [torch.empty_like(t) for t in (q, k, v)]
        Kk.attention_backward(q, k, v, out, dout, lse, *g, (False, False, False), H, False, 0.125)
        runs.append(g)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@functools.lru_cache(maxsize=None)
def _mha_model(dev, graph=False, B=16, T=48, E=64, heads=2, steps=3):
    """3 SGD steps of two blocks of causal self-attention + ReLU dense in fp32.  The projections carry
    no bias: the key bias has an exactly zero gradient (a softmax ignores a shift of its row), which a
    max-normalised comparison cannot scale."""
    from flexmi.core import ActiMode, FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = B, dev, "fp32", 5
    m = FFModel(cfg)
    x = h = m.create_tensor([B, T, E])
    for i in range(2):
        h = m.dense(m.multihead_attention(h, h, h, E, heads, bias=False, causal=True, name=f"mha{i}"), E, ActiMode.AC_MODE_RELU)
    m.dense(h, 1)
    # the loss sums over the T positions of a sample: a step size that keeps three steps stable
    m.compile(SGDOptimizer(m, 0.002), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(0)

    def feed():
        ex.scatter_from_host(x, rng.randn(B, T, E).astype(np.float32))
        ex.scatter_from_host(m.get_label_tensor(), rng.randn(B, T, 1).astype(np.float32))

    feed()
    ex.train_step()
    run = ex.capture_step() if graph else ex.train_step
    for _ in range(1, steps):
        feed()
        run()
    if dev == "gpu":
        torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters], m.get_perf_metrics().get_loss()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_mha_model_gpu_matches_cpu(gpu, graph):
    cpu, g = _mha_model("cpu"), _mha_model("gpu", graph)
    for a, b in zip(cpu[0], g[0]):
        assert np.abs(a - b).max() / max(np.abs(a).max(), 1e-6) < 1e-4, a.shape
    assert abs(cpu[1] - g[1]) < 1e-4 * max(1.0, abs(cpu[1]))
