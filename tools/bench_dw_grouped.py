#!/usr/bin/env python3
"""The top-MLP weight-gradient GEMMs of the MLPerf DLRM step (fp32, batch 8192: dW of 1024->512,
1024->1024 and 480->1024, each with its bias-gradient row sums) as three single launches + three
split-K reduces (what gemm() picks for each: tuned table, else the heuristic) against ONE grouped
launch + one reduce (gemm_grouped: the planner's depths, then forced depths 2 / 4 / 8).  Interleaved
rounds in one process, every call timed as 20 repeats captured in one hipGraph; prints one JSON line
per variant with the model's prediction beside the measurement.
usage: bench_dw_grouped.py [batch]"""
import json
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from flexmi.ops import _kernels as K  # noqa: E402
from tools.bench_gemm import timeit  # noqa: E402

LAYERS = [(1024, 512), (1024, 1024), (480, 1024)]      # (in, out) in backward order
# one 256x128 block: about 17 us + 0.0745 us per k of its K range (profiles/gemm_tune_candidates_r6.jsonl,
# dW orientation); a full-chip launch costs one block's time, a reduce about 8-11 us
T0_US, PER_K_US = 17.0, 0.0745


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ops = []
    for k, n in LAYERS:
        ops.append(dict(k=k, n=n, x=torch.randn(B, k, device=dev), dy=torch.randn(B, n, device=dev),
                        dw=torch.zeros(n, k, device=dev), db=torch.zeros(n, device=dev)))

    def singles():
        return [K.gemm(o["dy"], o["n"], False, o["x"], o["k"], False, o["dw"], o["k"], o["n"], o["k"], B, beta=True,
                       rowsum_a=o["db"]) for o in ops]

    def grouped(force):
        mem = [(o["dy"], o["n"], o["x"], o["k"], o["dw"], o["k"], o["n"], o["k"], B, True, o["db"]) for o in ops]
        return K.gemm_grouped(mem, False, False, force=force)

    variants = [("single_x3", singles)] + [(f"grouped_ks{f or 'plan'}", (lambda f=f: grouped(f))) for f in (0, 2, 4, 8)]
    depths = {name: fn() for name, fn in variants}
    if not all(depths["grouped_ksplan"]):
        print(json.dumps({"error": "the planner did not group these shapes", "depths": depths["grouped_ksplan"]}))
        return 1
    # the grouped result against the single launches (same accumulate-into-dW contract)
    for o in ops:
        o["dw"].zero_()
    singles()
    ref = [o["dw"].clone() for o in ops]
    for o in ops:
        o["dw"].zero_()
    grouped(0)
    err = max(((o["dw"] - r).abs().max() / r.abs().max()).item() for o, r in zip(ops, ref))
    best = {name: float("inf") for name, _ in variants}
    for _ in range(5):                                   # interleaved rounds
        for name, fn in variants:
            best[name] = min(best[name], timeit(fn) * 1e6)
    for name, _ in variants:
        ks = depths[name]
        if name == "single_x3":
            model = sum(T0_US + PER_K_US * B / d for d in ks) + 31.2     # the three measured reduces (prof_r7_final)
        else:
            blocks = sum(((n + 255) // 256) * ((k + 127) // 128) * d for (k, n), d in zip(LAYERS, ks))
            model = -(-blocks // 256) * (T0_US + PER_K_US * B / min(ks)) + 8.0      # waves of 256 blocks, one reduce
        print(json.dumps({"variant": name, "batch": B, "depths": ks, "us": round(best[name], 2), "model_us": round(model, 1),
                          "max_rel_diff_vs_single": err if name == "grouped_ksplan" else None}), flush=True)
    print(json.dumps({"single_us": round(best["single_x3"], 2), "grouped_us": round(best["grouped_ksplan"], 2),
                      "saved_us": round(best["single_x3"] - best["grouped_ksplan"], 2), "model_saved_us": 50.0}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
