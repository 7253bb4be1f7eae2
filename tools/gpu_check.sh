#!/bin/bash
# One GPU round: native-kernel tests, bench, optional conv microbench and rocprofv3 kernel stats.
# Each GPU step has its own timeout; steps are chained so a failure stops the script.
# Env knobs: STEPS, PROFILE=0|1, CONVBENCH=0|1, TESTS=0|1, OUT (output directory, default bench_out)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
STEPS=${STEPS:-20}
if [ "${TESTS:-1}" = "1" ]; then
  timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1; rc=$?
  tail -15 "$OUT/pytest_gpu.log"
  if [ $rc -ne 0 ] && [ $rc -ne 5 ]; then echo "pytest gpu failed rc=$rc"; exit $rc; fi
fi
if [ "${CONVBENCH:-0}" = "1" ]; then
  timeout -k 10 300 python tools/bench_conv.py --no-miopen > "$OUT/bench_conv.log" 2>&1 || { tail -20 "$OUT/bench_conv.log"; exit 1; }
  tail -1 "$OUT/bench_conv.log"
fi
# --full: the headline plus the per-phase timers and the fp32 record
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 5 > "$OUT/bench.log" 2>&1 || { tail -30 "$OUT/bench.log"; exit 1; }
tail -1 "$OUT/bench.log"
if [ "${PROFILE:-1}" = "1" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_bench" -o run -- python bench.py --full --steps 5 --warmup 3 > "$OUT/prof_bench.log" 2>&1 || { tail -20 "$OUT/prof_bench.log"; exit 1; }
  echo profiled
fi
