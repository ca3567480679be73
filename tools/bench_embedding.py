#!/usr/bin/env python3
"""Embedding-bag kernel microbenchmark (fused sparse-SGD backward and forward) over table
sizes of the MLPerf DLRM set: per-table time, effective bytes/s.  hipGraph of reps launches.

``--optimizer adagrad``: the grouped table backward of the 26 MLPerf tables (D = 128, batch 8192,
bf16 output gradients) under sparse Adagrad (fm_sdp_coalesce + fm_emb_adagrad_apply) and under the
sparse SGD the executor runs today (embedding_bwd_multi with its claim buffers), timed alternately
in the same process, each next to its byte model.  Uniformly drawn indices; tables above
``--max-rows`` rows are cut to that many (their lookups stay all but unique either way).

``--optimizer rowwise_adagrad``: the same A/B for row-wise Adagrad -- coalesce + row-wise apply
(fm_emb_rowwise_adagrad_apply) against coalesce + element-wise apply, alternated in one process.  Both share the coalesce, so the difference of two
timings is the difference of the applies; per-kernel times come from a kernel trace of the same
command."""
import argparse
import json
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from flexmi.ops import _kernels as K  # noqa: E402


def timed(fn, reps=20):
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(3):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


HBM_PEAK = 8.0e12   # B/s, MI355X


def adagrad_ab(B, max_rows, rounds, out):
    from flexmi.models.dlrm import MLPERF_TABLES
    from flexmi.ops.embedding import Embedding
    dev = torch.device("cuda")
    D = 128
    rows = [min(r, max_rows) for r in MLPERF_TABLES]
    lr = torch.tensor([0.01], device=dev)
    idx = [torch.randint(0, r, (B, 1), device=dev) for r in rows]
    dy = [(torch.randn(B, D, device=dev) * 1e-3).bfloat16() for _ in rows]
    ld = [d.stride(0) for d in dy]
    one, zero = [1.0] * len(rows), [0] * len(rows)
    U = sum(int(torch.unique(i).numel()) for i in idx)
    n = B * len(rows)

    def tables():
        return [torch.randn(r, D, device=dev) for r in rows]
    # sparse SGD as Embedding.backward_group runs it: claim buffers for the mostly-unique tables
    Ws = tables()
    claim = []
    for r in rows:
        if r > Embedding.CLAIM_RATIO * B:
            claim += [torch.full((r,), -1, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                      torch.zeros(1, dtype=torch.int32, device=dev)]
        else:
            claim += [None, None, None]

    def sgd():
        K.C().embedding_bwd_multi(Ws, idx, dy, ld, one, lr, claim, zero)
    # sparse Adagrad: coalesce into payloads, then the row updates of H and W
    Wa = tables()
    H = [torch.full((r, D), 0.1, device=dev) for r in rows]
    slot = [torch.full((r,), -1, dtype=torch.int32, device=dev) for r in rows]
    cid = [torch.empty(B, dtype=torch.int32, device=dev) for _ in rows]
    ids = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in rows]
    g = [torch.zeros(B * D, dtype=torch.float32, device=dev) for _ in rows]
    cnt = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in rows]

    def coalesce():
        K.C().sdp_coalesce(Wa, idx, dy, ld, one, zero, slot, cid, ids, g, cnt)

    def apply():
        K.C().emb_adagrad_apply(Wa, H, ids, g, cnt, slot, lr, 1e-10)

    def adagrad():
        coalesce()
        apply()
    # bytes the algorithms need, from the shapes (U unique rows of n lookups):
    #   sgd      : dy read + W read-modify-write per lookup, index reads
    #   coalesce : three index passes, slot claim / read, dy read, payload (g, ids, cid) write
    #   apply    : per unique row g read, H and W read-modify-write, ids read, slot release
    by = {"sgd": n * (D * 2 + 2 * D * 4 + 8),
          "coalesce": n * (3 * 8 + 2 * 4 + D * 2) + U * (D * 4 + 4 + 4),
          "apply": U * (D * 4 + 2 * D * 4 + 2 * D * 4 + 4 + 4)}
    by["adagrad"] = by["coalesce"] + by["apply"]
    t = {"sgd": [], "adagrad": []}
    for _ in range(rounds):                      # alternate the two forms: same neighbours, same clocks
        t["sgd"].append(timed(sgd))
        t["adagrad"].append(timed(adagrad))
    rec = {"B": B, "tables": len(rows), "D": D, "max_rows": max_rows, "lookups": n, "unique_rows": U}
    for k, v in t.items():
        best = min(v)
        rec[k] = {"us": round(best, 2), "us_all": [round(x, 2) for x in v], "model_bytes": by[k],
                  "GBps": round(by[k] / best / 1e3, 1), "of_hbm_peak": round(by[k] / (best * 1e-6) / HBM_PEAK, 3)}
    rec["model_bytes_coalesce"], rec["model_bytes_apply"] = by["coalesce"], by["apply"]
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def rowwise_ab(B, max_rows, rounds, out):
    from flexmi.models.dlrm import MLPERF_TABLES
    dev = torch.device("cuda")
    D = 128
    rows = [min(r, max_rows) for r in MLPERF_TABLES]
    lr = torch.tensor([0.01], device=dev)
    idx = [torch.randint(0, r, (B, 1), device=dev) for r in rows]
    dy = [(torch.randn(B, D, device=dev) * 1e-3).bfloat16() for _ in rows]
    ld = [d.stride(0) for d in dy]
    one, zero = [1.0] * len(rows), [0] * len(rows)
    U = sum(int(torch.unique(i).numel()) for i in idx)
    n = B * len(rows)
    # one table set and one coalesce buffer set for every form: same rows, same payloads
    W = [torch.randn(r, D, device=dev) for r in rows]
    H = [torch.full((r, D), 0.1, device=dev) for r in rows]
    h = [torch.full((r, 1), 0.1, device=dev) for r in rows]
    slot = [torch.full((r,), -1, dtype=torch.int32, device=dev) for r in rows]
    cid = [torch.empty(B, dtype=torch.int32, device=dev) for _ in rows]
    ids = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in rows]
    g = [torch.zeros(B * D, dtype=torch.float32, device=dev) for _ in rows]
    cnt = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in rows]

    def coalesce():
        K.C().sdp_coalesce(W, idx, dy, ld, one, zero, slot, cid, ids, g, cnt)

    def elementwise():
        coalesce()
        K.C().emb_adagrad_apply(W, H, ids, g, cnt, slot, lr, 1e-10)

    def rowwise():
        coalesce()
        K.C().emb_rowwise_adagrad_apply(W, h, ids, g, cnt, slot, lr, 1e-10)
    # bytes the applies need, from the shapes (U unique rows): g read, W read-modify-write, ids read,
    # slot release, and H read-modify-write (element-wise: D words; row-wise: one word)
    by = {"elementwise": U * (D * 4 + 2 * D * 4 + 2 * D * 4 + 4 + 4),
          "rowwise": U * (D * 4 + 2 * D * 4 + 2 * 4 + 4 + 4)}
    forms = {"elementwise": elementwise, "rowwise": rowwise}
    t = {k: [] for k in forms}
    for _ in range(rounds):                      # alternate the forms: same neighbours, same clocks
        for k, fn in forms.items():
            t[k].append(timed(fn))
    rec = {"B": B, "tables": len(rows), "D": D, "max_rows": max_rows, "lookups": n, "unique_rows": U,
           "model_bytes_apply": by}
    for k, v in t.items():
        rec[k] = {"coalesce_plus_apply_us": round(min(v), 2), "us_all": [round(x, 2) for x in v]}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", choices=["sgd", "adagrad", "rowwise_adagrad"], default="sgd")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--max-rows", type=int, default=4000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="append the result line to this file")
    a = ap.parse_args()
    if a.optimizer == "adagrad":
        return adagrad_ab(a.batch, a.max_rows, a.rounds, a.out)
    if a.optimizer == "rowwise_adagrad":
        return rowwise_ab(a.batch, a.max_rows, a.rounds, a.out)
    dev = torch.device("cuda")
    D = 128
    for B in (8192, 65536):
        for rows in (3, 4, 10, 36, 108, 155, 976, 7120, 39884406):
            W = torch.randn(rows, D, device=dev)
            idx = torch.randint(0, rows, (B, 1), device=dev)
            dy = (torch.randn(B, D, device=dev) * 1e-3).bfloat16()
            out = torch.empty(B, D, device=dev, dtype=torch.bfloat16)
            lr = torch.tensor([0.01], device=dev)
            tf = timed(lambda: K.embedding_forward(idx, W, out, 20))
            tb = timed(lambda: K.embedding_backward_sgd(idx, dy, W, lr, 20, {}))
            print(json.dumps({"B": B, "rows": rows, "fwd_us": round(tf, 2), "bwd_us": round(tb, 2),
                              "bwd_GBps": round(B * D * 2 / tb / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
