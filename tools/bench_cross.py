#!/usr/bin/env python3
"""A/B of the DCNv2 cross combine on MI355X: the fused ``cross.hip`` pass against the same result
composed from ``multiply`` + ``add`` (``elementwise.hip``), forward and backward.

    python tools/bench_cross.py [--out profiles/cross_ab.txt] [--rounds 7] [--reps 20]

Each variant's ``reps`` back-to-back launches are captured into one hipGraph (as
``flexmi/runtime/measure.py`` times an op); the variants are replayed in alternation, ``rounds``
times each in one process, and the median, minimum and maximum per-call times are reported with
the achieved bandwidth over the bytes each variant has to move (fused forward 4 tensors, composed
6; fused backward 7, composed 9 -- the three-input form with ``dx0`` accumulating and ``dx``
stored, as in a cross stack where every layer adds into the gradient of ``x_0``).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TBS = 6.3       # achievable HBM bandwidth of one MI355X (float4 copy)


def variants(shape, dtype, dev):
    import torch
    from flexmi.ops import _kernels as K
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda: torch.randn(shape, generator=g, device=dev).to(dtype)
    x0, t, x, dy = mk(), mk(), mk(), mk()
    y, prod, dprod, dt, dx0, dx = mk(), mk(), mk(), mk(), mk(), mk()

    def fused_fwd():
        K.cross_forward(x0, t, x, y)

    def comp_fwd():
        K.binary_forward(2, x0, t, prod)
        K.binary_forward(0, prod, x, y)

    def fused_bwd():
        K.cross_backward(dy, x0, t, dt, dx0, dx, False, True, False, False)

    def comp_bwd():
        K.binary_backward(0, prod, x, dy, dprod, dx, False, False)      # add: d(prod) = dy, dx = dy
        K.binary_backward(2, x0, t, dprod, dx0, dt, True, False)        # multiply: dx0 += d(prod) t, dt = d(prod) x0

    # tensors moved per call
    return [("fwd", "fused", fused_fwd, 4), ("fwd", "composed", comp_fwd, 6),
            ("bwd", "fused", fused_bwd, 7), ("bwd", "composed", comp_bwd, 9)]


def capture(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def replay_us(gr, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_cross needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_cross.py on {torch.cuda.get_device_name(0)}: {a.reps} launches per hipGraph, "
             f"{a.rounds} alternating replays per variant; us per call: median [min .. max]; roof {ROOF_TBS} TB/s",
             f"{'shape':<12}{'dtype':<6}{'pass':<5}{'variant':<10}{'us':>9}{'min':>9}{'max':>9}{'spread%':>9}"
             f"{'MB':>9}{'TB/s':>7}{'%roof':>7}{'fused/composed':>16}"]
    for shape in ((8192, 3456), (8192, 80)):
        for dtype in (torch.float32, torch.bfloat16):
            vs = variants(shape, dtype, dev)
            graphs = [capture(fn, a.reps) for _, _, fn, _ in vs]
            times = [[] for _ in vs]
            for _ in range(a.rounds):                        # alternate the variants within the session
                for k, gr in enumerate(graphs):
                    times[k].append(replay_us(gr, a.reps))
            med = [statistics.median(t) for t in times]
            for k, (ps, name, _, ntens) in enumerate(vs):
                mb = ntens * shape[0] * shape[1] * torch.empty(0, dtype=dtype).element_size() / 1e6
                tbs = mb / med[k]                            # MB / us = TB/s
                ratio = f"{med[k] / med[k + 1]:.3f}" if name == "fused" else ""
                lines.append(f"{'x'.join(map(str, shape)):<12}{'fp32' if dtype == torch.float32 else 'bf16':<6}{ps:<5}{name:<10}"
                             f"{med[k]:9.2f}{min(times[k]):9.2f}{max(times[k]):9.2f}"
                             f"{100 * (max(times[k]) - min(times[k])) / med[k]:9.1f}{mb:9.1f}{tbs:7.2f}"
                             f"{100 * tbs / ROOF_TBS:7.1f}{ratio:>16}")
            del graphs
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
