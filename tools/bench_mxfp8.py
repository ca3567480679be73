#!/usr/bin/env python3
"""Time the MXFP8 path against the bf16 Linear kernels on one GPU.

Per shape (rows x in x out): the MX GEMM alone and the whole pass with its quantisers, for the forward, dX and
dW, each next to the bf16 ``linear_forward`` / ``linear_backward`` phase it replaces.  Every candidate is
captured into a hipGraph of ``--inner`` calls; the graphs are replayed alternately ``--rounds`` times and the
median and the spread (min..max) of the per-call time are printed.  Output: one line per measurement.

Usage: python tools/bench_mxfp8.py [--rounds 7] [--inner 20] [--out profiles/mxfp8_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexmi.ops import _kernels as K  # noqa: E402

SHAPES = [(8192, 1024, 1024), (8192, 4096, 1024)]


def capture(fn, inner):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def candidates(M, Kd, N):
    dev, bf = "cuda", torch.bfloat16
    x, w = torch.randn(M, Kd, device=dev, dtype=bf), torch.randn(N, Kd, device=dev, dtype=bf) * 0.05
    b = torch.zeros(N, device=dev)
    y, dy = torch.empty(M, N, device=dev, dtype=bf), torch.randn(M, N, device=dev, dtype=bf)
    dx, dw, db = torch.empty(M, Kd, device=dev, dtype=bf), torch.zeros(N, Kd, device=dev), torch.zeros(N, device=dev)
    xq, wq, gq = K.mx_alloc(M, Kd, dev), K.mx_alloc(N, Kd, dev), K.mx_alloc(M, N, dev)
    K.mx_quant(x, 0, *xq)
    K.mx_quant(w, 0, *wq)
    K.linear_forward(x, w, b, 11, y)
    K.mx_quant_dact(dy, y, 11, *gq, db)
    ws = {}

    def bwd(phase):
        K.linear_backward(x, w, y, dy, 11, dx, False, dw, db, ws, False, None, phase, None)

    def mx_fwd_layer():
        K.mx_quant(x, 0, *xq)
        K.mx_quant(w, 0, *wq)
        K.mx_gemm(xq[0], xq[1], 0, wq[0], wq[1], 0, y, M, N, Kd, bias=b, act=11)

    def mx_dx_layer():
        K.mx_quant_dact(dy, y, 11, *gq, db)
        K.mx_gemm(gq[0], gq[1], 1, wq[2], wq[3], 0, dx, M, Kd, N)

    return {
        "fwd  bf16 linear_forward": lambda: K.linear_forward(x, w, b, 11, y),
        "fwd  mx gemm alone": lambda: K.mx_gemm(xq[0], xq[1], 0, wq[0], wq[1], 0, y, M, N, Kd, bias=b, act=11),
        "fwd  mx layer (2 quantisers + gemm)": mx_fwd_layer,
        "dX   bf16 linear_backward dx (act-bwd + gemm)": lambda: bwd("dx"),
        "dX   mx gemm alone": lambda: K.mx_gemm(gq[0], gq[1], 1, wq[2], wq[3], 0, dx, M, Kd, N),
        "dX   mx layer (quant_dact + gemm)": mx_dx_layer,
        "dW   bf16 linear_backward dw": lambda: bwd("dw"),
        "dW   mx gemm alone (= layer: copies exist)": lambda: K.mx_gemm(gq[2], gq[3], 1, xq[2], xq[3], 0, dw, N, Kd,
                                                                        (M + 127) // 128 * 128, beta=True),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mxfp8 needs a GPU"
    lines = []
    for M, Kd, N in SHAPES:
        cands = candidates(M, Kd, N)
        graphs = {k: capture(f, a.inner) for k, f in cands.items()}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():            # alternating: one replay of each per round
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                times[k].append(s.elapsed_time(e) * 1e3 / a.inner)
        flops = 2.0 * M * Kd * N
        for k, t in times.items():
            med = statistics.median(t)
            lines.append(f"{M}x{Kd}x{N}  {k:48s} {med:8.1f} us  (min {min(t):.1f} max {max(t):.1f})  "
                         f"{flops / med * 1e-6:7.1f} TFLOP/s of the product")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
