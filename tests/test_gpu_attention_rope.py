"""Rotary position embeddings fused into the attention kernels (csrc/kernels/attention.hip): the kernels
against a float64 oracle that rotates with a float64 table, rounds the rotated operands to storage where the
kernel does, and rotates the leaf gradients back; and a causal grouped-query encoder layer on the GPU
(eager and as a captured step) against the CPU backend."""
import functools

import numpy as np
import pytest
import torch

from tests.test_attention_rope_cpu import rotate_f64
from tests.test_gpu_attention import BWD_TOL, FWD_TOL, rel_err

pytestmark = pytest.mark.gpu
BASE = 10000.0


def _oracle(q, k, v, dout, H, KH, causal, lengths, inter):
    """float64 attention of the rotated operands rounded to storage (the one rounding the kernel adds), the
    gradients of those leaves rotated back in float64."""
    B, Tq, Tk, dh = q.shape[0], q.shape[1], k.shape[1], q.shape[2] // H
    sp = lambda t, n: t.double().reshape(B, t.shape[1], n, dh).transpose(1, 2)   # noqa: E731
    qr = rotate_f64(sp(q, H), BASE, inter).to(q.dtype).double().requires_grad_()
    kr = rotate_f64(sp(k, KH), BASE, inter).to(q.dtype).double().requires_grad_()
    vh = sp(v, KH).clone().requires_grad_()
    s = qr @ kr.repeat_interleave(H // KH, 1).transpose(-1, -2) * dh ** -0.5
    vis = torch.ones(Tq, Tk, dtype=torch.bool, device=q.device)
    vis = (vis.tril() if causal else vis)[None, None]
    if lengths is not None:
        vis = vis & (torch.arange(Tk, device=q.device)[None, :] < lengths.reshape(-1, 1))[:, None, None, :]
    out = (torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ vh.repeat_interleave(H // KH, 1)).transpose(1, 2)
    out = out.reshape(B, Tq, H * dh)
    out.backward(dout.double())
    back = lambda t: t.transpose(1, 2).reshape(B, t.shape[2], -1)   # noqa: E731
    return out.detach(), [back(rotate_f64(qr.grad, BASE, inter, True)), back(rotate_f64(kr.grad, BASE, inter, True)),
                          back(vh.grad)]


def _check(q, k, v, dout, grads, accs, H, KH, causal, lengths, inter, dt):
    from flexmi.ops import _kernels as Kk
    from flexmi.ops.attention import rope_table
    dh = q.shape[2] // H
    ref, dref = _oracle(q, k, v, dout, H, KH, causal, lengths, inter)
    tab = rope_table(max(q.shape[1], k.shape[1]), dh, BASE).to(q.device)
    out, lse = torch.full_like(q, 7.0), torch.empty(q.shape[0], H, q.shape[1], device=q.device)
    L = None if lengths is None else lengths.int()
    old = [g.double().clone() for g in grads]
    Kk.attention_forward(q, k, v, out, lse, H, causal, dh ** -0.5, KH, L, tab, inter)
    Kk.attention_backward(q, k, v, out, dout, lse, *grads, accs, H, causal, dh ** -0.5, KH, L, tab, inter)
    err = [rel_err(out, ref)] + [rel_err(g, d + (o if a else 0)) for g, d, o, a in zip(grads, dref, old, accs)]
    print("rel_err out, dq, dk, dv:", err)
    assert err[0] < FWD_TOL[dt] and max(err[1:]) < BWD_TOL[dt], err


# (B, H, KH, dh, Tq, Tk, causal, lengths, accumulate flags), each the smallest shape at which one part of the
# rotation can break: DH = 32 (one accumulator tile, partner g + 2) with a tail tile; a second bf16 key tile (a
# staged row's position is k0 + row); Tq != Tk with NT = 4, a table longer than Tq and several fp32 key tiles;
# shared forward / dQ blocks (positions follow qi), the dK/dV group loop, a second key block, a partly padded one.
CASES = [(2, 2, 2, 32, 33, 33, True, None, (True, False, False)), (1, 2, 2, 64, 70, 70, True, None, (False, True, False)),
         (1, 1, 1, 128, 40, 130, False, None, (False, False, True)),
         (2, 4, 2, 64, 130, 130, True, [130, 37], (False, False, False))]


@pytest.mark.parametrize("inter", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(x)) for x in c[:7]))
def test_rope_attention_vs_float64(gpu, case, dt, inter):
    B, H, KH, dh, Tq, Tk, causal, lengths, accs = case
    torch.manual_seed(11)
    q, k, v, dout = (torch.randn(B, T, n * dh, device=gpu).to(dt) for T, n in ((Tq, H), (Tk, KH), (Tk, KH), (Tq, H)))
    grads = [torch.randn_like(t) for t in (q, k, v)]
    _check(q, k, v, dout, grads, accs, H, KH, causal, None if lengths is None else torch.tensor(lengths, device=gpu),
           inter, dt)


@pytest.mark.parametrize("inter", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rope_attention_strided(gpu, dt, inter):
    """q/k/v and their gradients as column slices of [B, T, 3E] buffers; nothing outside the slices changes."""
    B, H, dh, T = 2, 2, 32, 70
    E = H * dh
    torch.manual_seed(12)
    qkv = torch.randn(B, T, 3 * E, device=gpu).to(dt)
    gbuf = torch.randn(B, T, 3 * E + 8, device=gpu).to(dt)
    keep_in, keep_pad = qkv.clone(), gbuf[:, :, 3 * E:].clone()
    _check(*(qkv[:, :, i * E:(i + 1) * E] for i in range(3)), torch.randn(B, T, E, device=gpu).to(dt),
           [gbuf[:, :, i * E:(i + 1) * E] for i in range(3)], (False, True, False), H, H, True, None, inter, dt)
    assert torch.equal(qkv, keep_in) and torch.equal(gbuf[:, :, 3 * E:], keep_pad)


@functools.lru_cache(maxsize=None)
def _encoder_model(dev, graph=False, B=8, T=40, E=64, heads=2, steps=3):
    """3 SGD steps of a causal grouped-query encoder layer with rotary positions in fp32, bias-free projections as in
    tests/test_gpu_attention.py."""
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = B, dev, "fp32", 5
    m = FFModel(cfg)
    x = m.create_tensor([B, T, E])
    h = m.transformer_encoder_layer(x, heads, 2 * E, causal=True, name="enc", attention_bias=False, num_kv_heads=1,
                                    rope_base=BASE)
    m.dense(h, 1)
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
def test_rope_encoder_gpu_matches_cpu(gpu, graph):
    cpu, g = _encoder_model("cpu"), _encoder_model("gpu", graph)
    errs = [np.abs(a - b).max() / max(np.abs(a).max(), 1e-6) for a, b in zip(cpu[0], g[0])]
    print("weights rel err:", max(errs), "loss:", cpu[1], g[1])
    assert max(errs) < 1e-4, errs
    assert abs(cpu[1] - g[1]) < 1e-4 * max(1.0, abs(cpu[1]))
