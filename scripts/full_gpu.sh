#!/bin/bash
# The GPU suite, then the full benchmark record (headline + every comparison run); logs go to $O.
set -e
O=${O:-results}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/gpu_suite.log 2>&1
timeout -k 10 600 python -u bench.py --full --steps 50 --warmup 10 > $O/bench_n1.jsonl 2> $O/bench_n1.err
