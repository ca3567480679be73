#!/usr/bin/env python3
"""A/B of the METRICS_AUC histogram kernel (csrc/kernels/auc.hip) on the GPU.

Times ``fm_auc_hist`` alone in three forms -- the shipped bounded peel ("bounded": a wave folds equal
keys into one atomic each until a few rounds found a key no other lane shares, then the other lanes
add 1 each), the full peel ("full_peel", 64 rounds) and one atomic per sample ("per_sample", 0
rounds) -- at B = 8192 and 65536 over four score sets: all scores equal, eight values drawn at
random (16 hot keys), bf16-rounded logistic scores, and distinct fp32 scores.  Each sample is the
device-event time of ``--launches`` back-to-back launches divided by their number; the variants
alternate sample by sample, and the table gives the median and the spread of ``--samples`` samples
after a warm-up.  All variants must leave the same histogram.

    python tools/bench_auc.py [--out profiles/auc_hist_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


VARIANTS = {"bounded": -1, "full_peel": 64, "per_sample": 0}      # name -> peel rounds (-1: the shipped default)


def score_sets(n, torch):
    g = torch.Generator().manual_seed(7)
    y = (torch.rand(n, generator=g) < 0.25).float()
    z = torch.randn(n, generator=g) * 1.5 + y - 2.0
    p = torch.sigmoid(z)
    distinct = torch.linspace(0.01, 0.99, n)           # n distinct fp32 values: no two lanes share a key
    eight = torch.randint(0, 8, (n,), generator=g).float() / 16 + 0.25      # 8 bins x 2 classes = 16 hot keys
    return {"all_equal": (torch.full((n,), 0.5), y), "eight_values": (eight, y), "logistic_bf16": (p.bfloat16(), y),
            "distinct_fp32": (distinct, y)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_auc: needs a GPU")
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT
    from flexmi.ops import _kernels as K
    dev = torch.device("cuda", 0)
    lines = [f"fm_auc_hist A/B, shift {AUC_SHIFT}: us per launch, median [min, max] of {a.samples} samples of "
             f"{a.launches} launches, variants alternating",
             f"{'B':>7} {'scores':<14} " + " ".join(f"{v:>24}" for v in VARIANTS)]
    for n in [int(v) for v in a.sizes.split(",")]:
        for name, (s, y) in score_sets(n, torch).items():
            s, y = s.to(dev).reshape(n, 1), y.to(dev).reshape(n, 1)
            hists = {}
            for v, rounds in VARIANTS.items():
                h = torch.zeros(2, AUC_BINS, dtype=torch.int64, device=dev)
                iv = torch.zeros(1, dtype=torch.int64, device=dev)
                K.auc_hist(s, y, h, iv, AUC_SHIFT, rounds=rounds)
                hists[v] = h
            if any(not torch.equal(hists["bounded"], h) for h in hists.values()) or int(hists["bounded"].sum()) != n:
                raise SystemExit(f"bench_auc: variants disagree at B={n} {name}")
            h, iv = hists["bounded"], torch.zeros(1, dtype=torch.int64, device=dev)
            for rounds in VARIANTS.values():
                for _ in range(a.warmup):
                    K.auc_hist(s, y, h, iv, AUC_SHIFT, rounds=rounds)
            torch.cuda.synchronize()
            t = {v: [] for v in VARIANTS}
            for _ in range(a.samples):
                for v, rounds in VARIANTS.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        K.auc_hist(s, y, h, iv, AUC_SHIFT, rounds=rounds)
                    e1.record()
                    e1.synchronize()
                    t[v].append(e0.elapsed_time(e1) * 1e3 / a.launches)
            cell = [f"{statistics.median(x):8.2f} [{min(x):6.2f},{max(x):7.2f}]" for x in t.values()]
            lines.append(f"{n:>7} {name:<14} " + " ".join(f"{c:>24}" for c in cell))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
