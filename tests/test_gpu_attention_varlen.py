"""Fused attention with per-sample key lengths and grouped-query heads (csrc/kernels/attention.hip)
against the float64 oracle of tests/test_attention_varlen_cpu.py, NaN in every padded key row; the
grouped dK/dV sum run twice; an MQA model with changing lengths, eager and captured, against the CPU."""
import numpy as np
import pytest
import torch

from tests.test_attention_varlen_cpu import oracle, rel_err, train
from tests.test_gpu_attention import BWD_TOL, FWD_TOL

pytestmark = pytest.mark.gpu

# (B, heads, kv_heads, dh, Tq, Tk, causal, lengths, accumulate flags, pad): empty row / one key / tile edge / full; dK/dV
# blocks wholly and partly past the length; length and diagonal in one loop; G = 4; G = 3; all at once on column slices
NOACC = (False, False, False)
CASES = [(4, 2, 2, 32, 33, 70, False, [0, 1, 64, 70], NOACC, 0), (3, 1, 1, 64, 40, 200, False, [5, 129, 200], NOACC, 0),
         (3, 2, 2, 64, 130, 130, True, [1, 65, 130], NOACC, 0), (2, 4, 1, 64, 33, 70, False, None, NOACC, 0),
         (2, 6, 2, 32, 200, 17, False, None, NOACC, 0), (2, 4, 2, 128, 130, 130, True, [7, 130], (True, False, True), 16)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(x)) for x in c[:7]) + f"_{c[7]}")
def test_varlen_gqa_vs_float64(gpu, case, dt):
    from flexmi.ops import _kernels as Kk
    B, H, KH, dh, Tq, Tk, causal, lens, accs, pad = case
    torch.manual_seed(11)
    mk = lambda T, n: torch.randn(B, T, n * dh + 2 * pad, device=gpu).to(dt)[:, :, pad:pad + n * dh]   # noqa: E731
    q, k, v, dout, out = mk(Tq, H), mk(Tk, KH), mk(Tk, KH), mk(Tq, H), mk(Tq, H)
    L = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=gpu).reshape(B, 1)
    dead = torch.arange(Tk, device=gpu)[None] >= (torch.full((B, 1), Tk, device=gpu) if L is None else L)
    ref, dref = oracle(q, k, v, dout, H, KH, causal, L)
    k[dead], v[dead] = float("nan"), float("nan")
    lse = torch.empty(B, H, Tq, device=gpu)
    for absent in ((None, 1) if pad else (None,)):
        grads = [None if i == absent else mk(T, n) for i, (T, n) in enumerate(((Tq, H), (Tk, KH), (Tk, KH)))]
        old = [None if g is None else g.clone() for g in grads]
        Kk.attention_forward(q, k, v, out, lse, H, causal, dh ** -0.5, KH, L)
        Kk.attention_backward(q, k, v, out, dout, lse, *grads, accs, H, causal, dh ** -0.5, KH, L)
        err = [rel_err(out, ref)]
        assert torch.isfinite(out).all() and (lens is None or 0 not in lens or (out[lens.index(0)] == 0).all())
        for i, (g, d, o, a) in enumerate(zip(grads, dref, old, accs)):
            if g is None:
                continue
            if i:                                                # padded rows exactly, then the visible ones
                assert torch.equal(g[dead], o[dead] if a else torch.zeros_like(o[dead])), i
                g, d, o = g[~dead], d[~dead], o[~dead]
            assert torch.isfinite(g).all(), i
            err.append(rel_err(g, d + (o if a else 0)))
        print("rel_err out, grads:", err)
        assert err[0] < FWD_TOL[dt] and max(err[1:]) < BWD_TOL[dt], err


def test_grouped_backward_is_deterministic(gpu):
    from flexmi.ops import _kernels as Kk
    B, H, KH, dh, Tq, Tk = CASES[3][:6]
    torch.manual_seed(9)
    q, k, v = (torch.randn(B, T, n * dh, device=gpu).bfloat16() for T, n in ((Tq, H), (Tk, KH), (Tk, KH)))
    out, dout, lse = torch.empty_like(q), torch.randn_like(q), torch.empty(B, H, Tq, device=gpu)
    Kk.attention_forward(q, k, v, out, lse, H, False, 0.125, KH)
    runs = []
    for _ in range(2):
        runs.append([torch.empty_like(t) for t in (q, k, v)])
        Kk.attention_backward(q, k, v, out, dout, lse, *runs[-1], NOACC, H, False, 0.125, KH)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_mqa_model_with_lengths_gpu_matches_cpu(gpu, graph):
    """The captured run is the check that the lengths are read at replay time: they change every step."""
    cpu, g = train("cpu"), train("gpu", graph)
    for a, b in zip(cpu[0], g[0]):
        assert np.abs(a - b).max() / max(np.abs(a).max(), 1e-6) < 1e-4, a.shape
    assert abs(cpu[1] - g[1]) < 1e-4 * max(1.0, abs(cpu[1]))
