#!/usr/bin/env python3
"""Time the gated feed-forward (SwiGLU) kernels on one GPU: the fused forward (csrc/kernels/glu.hip) against the
composed one (the Linear GEMM with N = 2F, then fm_glu_act_fwd), and the whole forward + backward with either.

Per shape (rows M, in H, out F) every candidate is captured into a hipGraph of ``--inner`` calls; the graphs are
replayed alternately ``--rounds`` times and the median and the spread (min..max) of the per-call time are printed,
with TFLOP/s over the forward product ``2 M H 2F`` (three times that for forward + backward).

Usage: python tools/bench_glu.py [--rounds 7] [--inner 10] [--out profiles/glu_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexmi.ops import _kernels as K  # noqa: E402

SHAPES = [(8192, 1024, 2816), (8192, 1024, 4096), (4096, 4096, 11008)]


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
    x, w = torch.randn(M, H, device=dev, dtype=bf), torch.randn(2 * F, H, device=dev, dtype=bf) * H ** -0.5
    gu, h = torch.empty(M, 2 * F, device=dev, dtype=bf), torch.empty(M, F, device=dev, dtype=bf)
    dh, dgu = torch.randn(M, F, device=dev, dtype=bf), torch.empty(M, 2 * F, device=dev, dtype=bf)
    dx, dw = torch.empty(M, H, device=dev, dtype=bf), torch.zeros(2 * F, H, device=dev)
    assert K.glu_gemm_eligible(x, w, gu, h)

    def fused():
        K.glu_gemm_fwd(x, w, gu, h, 0)

    def gemm2f():
        K.gemm(x, H, True, w, H, True, gu, 2 * F, M, 2 * F, H)

    def composed():
        gemm2f()
        K.glu_act_fwd(gu, h, 0)

    def backward():
        K.glu_act_bwd(dh, gu, dgu, 0)
        K.gemm(dgu, 2 * F, True, w, H, False, dx, H, M, H, 2 * F)
        K.gemm(dgu, 2 * F, False, x, H, False, dw, H, 2 * F, H, M, beta=True)

    return {
        "fwd      fused (one kernel)": (fused, 1),
        "fwd      composed (gemm N=2F + act_fwd)": (composed, 1),
        "fwd      composed: its gemm alone": (gemm2f, 1),
        "fwd+bwd  fused forward": (lambda: (fused(), backward()), 3),
        "fwd+bwd  composed forward": (lambda: (composed(), backward()), 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_glu needs a GPU"
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
            flops = 2.0 * M * H * 2 * F * cands[k][1]
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
