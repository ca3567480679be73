#!/usr/bin/env python3
"""A/B of the embedding forward for tables of unequal bag sizes: the per-table-grid kernels
(``embedding_set_fwd_mode(1)``: fm_emb_fwd_multi, every table the same grid) against the work-balanced
kernel (mode 2: fm_emb_fwd_balanced, blocks dealt out in proportion to each table's lookups).

Shapes: ``mlperf`` = the 26 MLPerf tables with the per-table multi-hot sizes (214 lookups per sample),
D = 128, fp32 tables above ``--max-rows`` rows cut to that many; ``tiny`` = tiny_dcn_multihot's four
tables (D = 16, bags 3-1-8-2), the launch-bound end.  Uniformly drawn int64 indices, fp32 and bf16
outputs.  Each form is a hipGraph of ``--reps`` launches timed with device events; the forms alternate
in one process for ``--rounds`` rounds and every round's time is printed, so the spread is visible.
Beside each time: the bytes the algorithm needs (rows read + indices read + outputs written, from the
shapes) and the rate they give.  Before timing, the two forms' outputs are compared bit for bit."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexmi.models.dlrm import MLPERF_MULTIHOT_SIZES, MLPERF_TABLES, DLRMConfig  # noqa: E402
from flexmi.ops import _kernels as K  # noqa: E402

HBM_PEAK = 8.0e12   # B/s, MI355X


def capture(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run(shape, B, out_dt, a):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if shape == "mlperf":
        rows, bags, D = [min(r, a.max_rows) for r in MLPERF_TABLES], list(MLPERF_MULTIHOT_SIZES), 128
    else:
        c = DLRMConfig.preset("tiny_dcn_multihot")
        rows, bags, D = list(c.embedding_size), c.bag_sizes(), c.sparse_feature_size
    W = [torch.randn(r, D, device=dev) for r in rows]
    idx = [torch.randint(0, r, (B, b), device=dev) for r, b in zip(rows, bags)]
    esz = 4 if out_dt == torch.float32 else 2
    nbytes = sum(B * b * (D * 4 + 8) + B * D * esz for b in bags)
    row_bytes = sum(B * b * D * 4 for b in bags)

    def form(mode):
        outs = [torch.empty(B, D, device=dev, dtype=out_dt) for _ in rows]

        def fn():
            K.C().embedding_fwd_multi(W, idx, outs, [D] * len(rows), [1.0] * len(rows))
        K.embedding_set_fwd_mode(mode)
        g = capture(fn, a.reps)                    # the mode is read at launch, i.e. at capture
        name = K.embedding_fwd_last_form()
        K.embedding_set_fwd_mode(0)
        return g, outs, name

    forms = {"table_grid": form(1), "balanced": form(2)}
    assert forms["table_grid"][2] in ("multi", "multi_su") and forms["balanced"][2] == "balanced", forms
    ref = forms["table_grid"][1]
    for name, (g, outs, _) in forms.items():
        assert all(torch.equal(x, y) for x, y in zip(outs, ref)), f"{name}: outputs differ from the table-grid kernel"
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, (g, _, _) in forms.items():
            times[k].append(time_us(g, a.reps))
    res = {"shape": shape, "B": B, "tables": len(rows), "D": D, "out": str(out_dt).split(".")[1], "lookups_per_sample": sum(bags),
           "row_bytes": row_bytes, "model_bytes": nbytes, "reps": a.reps}
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                  "us_all": [round(x, 2) for x in t], "TBps": round(nbytes / med / 1e6, 3),
                  "of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["mlperf", "tiny"], default="mlperf")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--max-rows", type=int, default=4000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_emb_multihot.py needs a GPU")
    torch.cuda.set_device(0)
    for out_dt in (torch.float32, torch.bfloat16):
        run(a.shape, a.batch, out_dt, a)


if __name__ == "__main__":
    main()
