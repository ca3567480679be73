#!/usr/bin/env python3
"""Timing of the fused LayerNorm kernels (``csrc/kernels/layernorm.hip``) on MI355X, forward and
backward, with and without the fused residual, in bf16 and fp32, against a yardstick timed in the
same session: the streaming ``fm_cross_fwd`` / ``fm_cross_bwd`` kernels at the same element count.

    python tools/bench_layernorm.py [--out profiles/layernorm.txt] [--rounds 7] [--reps 20]

Each variant's ``reps`` back-to-back launches are captured into one hipGraph; the variants of a shape
and dtype are replayed in alternation, ``rounds`` times each, and the median, minimum and maximum
per-call times are reported with the bandwidth over the bytes the variant has to move, computed from
the shapes: LayerNorm forward x (+ residual) and y; backward x (+ residual), dy, dx (+ dresidual);
cross forward 4 tensors, backward 7.  The row statistics, weights and partial sums are not counted.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_cross import ROOF_TBS, capture, replay_us   # noqa: E402

SHAPES = ((65536, 128), (16384, 1024), (8192, 3456))


def variants(shape, dtype, dev):
    import torch
    from flexmi.ops import _kernels as K
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda: torch.randn(shape, generator=g, device=dev).to(dtype)   # noqa: E731
    x, r, y, dy, dx, dr, t = mk(), mk(), mk(), mk(), mk(), mk(), mk()
    gamma, beta = torch.ones(shape[1], device=dev), torch.zeros(shape[1], device=dev)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(beta)
    stats = torch.empty(shape[0], 2, device=dev)
    out = []
    for res, n_f, n_b in ((None, 2, 3), (r, 3, 5)):
        tag = "ln" if res is None else "ln+res"
        out.append(("fwd", tag, lambda res=res: K.layernorm_forward(x, res, y, gamma, beta, stats, 1e-5, False), n_f))
        out.append(("bwd", tag, lambda res=res: K.layernorm_backward(x, res, dy, gamma, stats, dx, None if res is None else dr,
                                                                     False, False, dgamma, dbeta, False), n_b))
    out.append(("fwd", "cross", lambda: K.cross_forward(x, t, r, y), 4))
    out.append(("bwd", "cross", lambda: K.cross_backward(dy, x, t, dx, dr, y, False, True, False, False), 7))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_layernorm needs a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_layernorm.py on {torch.cuda.get_device_name(0)}: {a.reps} launches per hipGraph, "
             f"{a.rounds} alternating replays per variant; us per call: median [min .. max]; roof {ROOF_TBS} TB/s",
             f"{'shape':<12}{'dtype':<6}{'pass':<5}{'variant':<8}{'us':>9}{'min':>9}{'max':>9}{'spread%':>9}{'MB':>9}"
             f"{'TB/s':>7}{'%roof':>7}{'rate/cross':>12}"]
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            vs = variants(shape, dtype, dev)
            graphs = [capture(fn, a.reps) for _, _, fn, _ in vs]
            times = [[] for _ in vs]
            for _ in range(a.rounds):                        # alternate the variants within the session
                for k, gr in enumerate(graphs):
                    times[k].append(replay_us(gr, a.reps))
            med = [statistics.median(t) for t in times]
            mbs = [n * shape[0] * shape[1] * torch.empty(0, dtype=dtype).element_size() / 1e6 for _, _, _, n in vs]
            rate = {(ps, name): mbs[k] / med[k] for k, (ps, name, _, _) in enumerate(vs)}   # MB / us = TB/s
            for k, (ps, name, _, _) in enumerate(vs):
                tbs = rate[(ps, name)]
                lines.append(f"{'x'.join(map(str, shape)):<12}{'fp32' if dtype == torch.float32 else 'bf16':<6}{ps:<5}{name:<8}"
                             f"{med[k]:9.2f}{min(times[k]):9.2f}{max(times[k]):9.2f}"
                             f"{100 * (max(times[k]) - min(times[k])) / med[k]:9.1f}{mbs[k]:9.1f}{tbs:7.2f}"
                             f"{100 * tbs / ROOF_TBS:7.1f}{tbs / rate[(ps, 'cross')]:12.2f}")
            del graphs
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
