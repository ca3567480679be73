#!/usr/bin/env python3
"""Time the dense + GELU / SiLU kernels on one GPU: the fused forward (csrc/kernels/act_gemm.hip) with either block tile
against the composed one (the Linear GEMM with its bias epilogue into pre, then the unary kernel), and forward + backward of
an ActLinear against a Linear with ReLU of the same shape (the price of the kept pre-activation).

Per shape (rows M, in H, out F) every candidate is captured into a hipGraph of ``--inner`` calls; the graphs are replayed
alternately ``--rounds`` times and the median and the spread (min..max) of the per-call time are printed, with TFLOP/s over
the forward product ``2 M H F`` (three times that for forward + backward).

Usage: python tools/bench_act_linear.py [--rounds 7] [--inner 10] [--out profiles/act_linear_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexmi.ops import _kernels as K  # noqa: E402

SHAPES = [(8192, 1024, 2816), (8192, 1024, 4096), (4096, 4096, 11008)]
CODES = {"gelu": 5, "silu": 7}
RELU, NONE = 11, 10


def capture(fn, inner):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def candidates(M, H, F):
    dev, bf = "cuda", torch.bfloat16
    x, w = torch.randn(M, H, device=dev, dtype=bf), torch.randn(F, H, device=dev, dtype=bf) * H ** -0.5
    b, db = torch.randn(F, device=dev), torch.zeros(F, device=dev)
    pre, y = torch.empty(M, F, device=dev, dtype=bf), torch.empty(M, F, device=dev, dtype=bf)
    dy, dpre = torch.randn(M, F, device=dev, dtype=bf), torch.empty(M, F, device=dev, dtype=bf)
    dx, dw, ws = torch.empty(M, H, device=dev, dtype=bf), torch.zeros(F, H, device=dev), {}
    assert K.act_gemm_eligible(x, w, b, pre, y)

    def fused(code, tile):
        return lambda: K.act_gemm_fwd(x, w, b, pre, y, code, tile)

    def gemm_bias():
        K.linear_forward(x, w, b, NONE, pre)

    def composed(code):
        return lambda: (gemm_bias(), K.unary_forward(code, pre, y))

    def act_backward(code):
        K.act_bwd(dy, pre, dpre, db, code)
        K.linear_backward(x, w, dpre, dpre, NONE, dx, False, dw, None, ws)

    def relu_layer():
        K.linear_forward(x, w, b, RELU, y)
        K.linear_backward(x, w, y, dy, RELU, dx, False, dw, db, ws)

    c = {}
    for name, code in CODES.items():
        c[f"fwd      {name} fused, tile 128"] = (fused(code, 128), 1)
        c[f"fwd      {name} fused, tile 64"] = (fused(code, 64), 1)
        c[f"fwd      {name} composed (gemm + unary)"] = (composed(code), 1)
    c["fwd      composed: its gemm alone"] = (gemm_bias, 1)
    c["fwd+bwd  ActLinear gelu, fused tile 128"] = (lambda: (fused(5, 128)(), act_backward(5)), 3)
    c["fwd+bwd  ActLinear gelu, composed"] = (lambda: (composed(5)(), act_backward(5)), 3)
    c["fwd+bwd  Linear relu"] = (relu_layer, 3)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_act_linear needs a GPU"
    lines = []
    for M, H, F in SHAPES:
        cands = candidates(M, H, F)
        graphs = {k: capture(f, a.inner) for k, (f, _) in cands.items()}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():            # alternating: one replay of each per round
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                times[k].append(s.elapsed_time(e) * 1e3 / a.inner)
        for k, t in times.items():
            med = statistics.median(t)
            flops = 2.0 * M * H * F * cands[k][1]
            lines.append(f"M={M} H={H} F={F}  {k:42s} {med:9.1f} us  (min {min(t):.1f} max {max(t):.1f})  "
                         f"{flops / med * 1e-6:7.1f} TFLOP/s")
        del graphs, cands
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
