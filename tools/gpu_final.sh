#!/bin/bash
# Round-end evidence in one call: GPU tests, the full C3 bench (CPU baseline,
# whole-batch parity, C3J, widened rows), a kernel-trace profile of the
# bench, the PMC passes, the per-eval select profile and the host-stage
# probe.  Each GPU step under its own limit, chained: stop at the first failure.
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}  # where logs and results go (tools/pmc.sh below writes there too)
mkdir -p "$OUT"
if [ -n "$RUN_TESTS" ]; then  # the whole GPU suite takes ~10 min: usually a call of its own
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 600 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo TESTS_FAILED; tail -30 $OUT/gpu_tests.log; exit 1; }
  tail -2 $OUT/gpu_tests.log
fi
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAILED; tail -5 $OUT/bench.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/bench.json')); print(d['value'], d['stages'], d['roofline']['frac'], d['parity_full_batch'], d['extras']['c3j'])"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --full --no-cpu --no-extras > $OUT/prof_bench.json 2> $OUT/prof.log || { echo PROF_FAILED; exit 1; }
bash tools/pmc.sh || { echo PMC_FAILED; exit 1; }
timeout -k 10 150 python tools/probe_join.py --reps 3 > $OUT/probe_join.log 2>&1 || { echo JOIN_PROBE_FAILED; exit 1; }
timeout -k 10 200 python tools/probe_host.py > $OUT/probe_host.log 2>&1 || { echo HOST_PROBE_FAILED; exit 1; }
cat $OUT/probe_host.log
echo rc=0
