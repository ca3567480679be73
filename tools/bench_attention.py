#!/usr/bin/env python3
"""Timing of the fused attention kernels (``csrc/kernels/attention.hip``) on MI355X against the same
forward composed from the project's ``bmm`` + ``softmax`` + ``bmm``.

    python tools/bench_attention.py [--out profiles/attention.txt] [--rounds 5] [--reps 4] [--quick]
                                    [--kv-heads N] [--mean-length M] [--rope half|interleaved]

``B = 32, heads = 8, dh in {64, 128}, T in {512, 2048}``, causal and not, bf16 and fp32.  Each
variant's ``reps`` back-to-back calls are captured into one hipGraph; the variants of one shape are
replayed in alternation, ``rounds`` times each in one process, and the median per-call time is
reported with its spread and the achieved TF/s over the algorithmic flops (4 B heads T^2 dh forward,
2.5x that backward, halved when causal).  The composition works on head-major ``[B heads, T, dh]``
copies made outside the timing, writes the ``[B heads, T, T]`` scores to memory, applies no mask (it
does the non-causal work in either case) and has no backward: the project's softmax backward is the
identity, which is why the fused op exists.

``--kv-heads N`` gives ``k`` / ``v`` (and ``dk`` / ``dv``) ``N`` heads (grouped-query attention);
``--mean-length M`` gives every sample a key length drawn uniformly from ``M - w .. M + w``, ``w = min(M,
T - M)``, with a fixed seed (a ``T`` below ``M`` is skipped).  Either drops the composition, which can do neither, and TF/s stays over
the flops of the full-length problem, so that a time saved shows as a higher figure.
``--rope half|interleaved`` rotates ``q`` and ``k`` in the kernels (rotary position embedding, base 10000); it drops
the composition as well, and TF/s stays over the flops of the products alone.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_cross import capture, replay_us  # noqa: E402


def variants(B, H, dh, T, causal, dtype, dev, kv_heads=None, mean_length=None, rope=None):
    import torch
    from flexmi.ops import _kernels as K
    g = torch.Generator(device=dev).manual_seed(0)
    KH = kv_heads or H
    mk = lambda n=H: torch.randn(B, T, n * dh, generator=g, device=dev).to(dtype)   # noqa: E731
    q, k, v, dout, out, dq, dk, dv = (mk(n) for n in (H, KH, KH, H, H, H, KH, KH))
    lens = None
    if mean_length is not None:
        w = min(mean_length, T - mean_length)
        lens = torch.randint(mean_length - w, mean_length + w + 1, (B, 1), generator=g, device=dev).int()
    lse = torch.empty(B, H, T, device=dev)
    tab = None
    if rope is not None:
        from flexmi.ops.attention import rope_table
        tab = rope_table(T, dh, 10000.0).to(dev)
    inter = rope == "interleaved"
    scale = dh ** -0.5

    def fused_fwd():
        K.attention_forward(q, k, v, out, lse, H, causal, scale, KH, lens, tab, inter)

    def fused_bwd():
        K.attention_backward(q, k, v, out, dout, lse, dq, dk, dv, (False, False, False), H, causal, scale, KH, lens, tab,
                             inter)

    fl = 4.0 * B * H * T * T * dh * (0.5 if causal else 1.0)
    if KH != H or lens is not None or tab is not None:
        return [("fwd", "fused", fused_fwd, fl), ("bwd", "fused", fused_bwd, 2.5 * fl)]
    hm = lambda t: t.reshape(B, T, H, dh).transpose(1, 2).reshape(B * H, T, dh).contiguous()   # noqa: E731
    qh, kh, vh = hm(q * scale), hm(k), hm(v)
    s = torch.empty(B * H, T, T, device=dev, dtype=dtype)
    p = torch.empty_like(s)
    oh = torch.empty_like(qh)

    def composed_fwd():
        K.bmm(qh, kh, s, False, True, False)
        K.softmax_forward(s, p)
        K.bmm(p, vh, oh, False, False, False)

    return [("fwd", "fused", fused_fwd, fl), ("fwd", "composed", composed_fwd, fl), ("bwd", "fused", fused_bwd, 2.5 * fl)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--quick", action="store_true", help="T = 512 only")
    ap.add_argument("--kv-heads", type=int, default=None, help="heads of k / v (default: all 8)")
    ap.add_argument("--mean-length", type=int, default=None, help="mean of the per-sample key lengths (default: none given)")
    ap.add_argument("--rope", choices=("half", "interleaved"), default=None, help="rotary position embedding of q and k")
    ap.add_argument("--long", action="store_true", help="T = 2048 only")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_attention needs a GPU"
    dev = torch.device("cuda", 0)
    B, H = 32, 8
    lines = [f"# tools/bench_attention.py on {torch.cuda.get_device_name(0)}: B={B} heads={H} kv_heads={a.kv_heads or H} "
             f"mean_length={a.mean_length} rope={a.rope}, {a.reps} calls per hipGraph, "
             f"{a.rounds} alternating replays per variant; us per call: median [min .. max]; TF/s over algorithmic flops",
             f"{'dh':>4}{'T':>6}{'causal':>7} {'dtype':<6}{'pass':<5}{'variant':<10}{'us':>10}{'min':>10}{'max':>10}{'TF/s':>8}"
             f"{'fused/composed':>16}"]
    for dh in (64, 128):
        for T in ((512,) if a.quick else (2048,) if a.long else (512, 2048)):
            if a.mean_length is not None and a.mean_length > T:
                continue
            for causal in (False, True):
                for dtype in (torch.bfloat16, torch.float32):
                    vs = variants(B, H, dh, T, causal, dtype, dev, a.kv_heads, a.mean_length, a.rope)
                    graphs = [capture(fn, a.reps) for _, _, fn, _ in vs]
                    times = [[] for _ in vs]
                    for _ in range(a.rounds):                # alternate the variants within the session
                        for i, gr in enumerate(graphs):
                            times[i].append(replay_us(gr, a.reps))
                    med = [statistics.median(t) for t in times]
                    for i, (ps, name, _, fl) in enumerate(vs):
                        ratio = f"{med[0] / med[1]:.3f}" if (ps, name) == ("fwd", "fused") and len(vs) == 3 else ""
                        lines.append(f"{dh:>4}{T:>6}{str(causal):>7} {'fp32' if dtype == torch.float32 else 'bf16':<6}{ps:<5}"
                                     f"{name:<10}{med[i]:10.1f}{min(times[i]):10.1f}{max(times[i]):10.1f}"
                                     f"{fl / med[i] / 1e6:8.1f}{ratio:>16}")
                    del graphs, vs
                    torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
