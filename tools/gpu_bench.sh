#!/bin/bash
# Quick C3 bench only (no CPU leg, no extras): value and stage times.
export TMPDIR=/tmp
OUT=${OUT:-bench_out}  # where logs and results go
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full --no-cpu --no-extras "$@" > $OUT/bench_quick.json 2> $OUT/bench_quick.err || { echo BENCH_FAILED; tail -5 $OUT/bench_quick.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/bench_quick.json')); print(d['value'], d['step_ms'], d['stages'], d['roofline']['frac'], d['host'])"
echo rc=0
