#!/bin/bash
# GPU-box session: parity tests, then (only if no crash) a short bench and a rocprofv3 summary.
# Each GPU step has its own time limit; any abort/segfault/timeout ends the script.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}  # where this script writes its logs and results
mkdir -p $OUT
export TMPDIR=/tmp
ok_or_stop() {  # rc 0 = pass, 1 = test failures (still safe to continue); anything else stops
  local rc=$1 what=$2
  echo "[$what] rc=$rc"
  if [ "$rc" -ne 0 ] && [ "$rc" -ne 1 ]; then echo "stopping after $what (rc=$rc)"; exit "$rc"; fi
}
STAGE=${1:-all}
if [ "$STAGE" = all ] || [ "$STAGE" = test ]; then
  timeout -k 10 ${TEST_TIMEOUT:-900} python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread ${PYTEST_ARGS} > $OUT/pytest_gpu.log 2>&1
  ok_or_stop $? pytest
  tail -5 $OUT/pytest_gpu.log
fi
if [ "$STAGE" = all ] || [ "$STAGE" = bench ]; then
  timeout -k 10 ${BENCH_TIMEOUT:-400} python bench.py --full ${BENCH_ARGS} > $OUT/bench.log 2>&1
  ok_or_stop $? bench
  tail -2 $OUT/bench.log
fi
if [ "$STAGE" = all ] || [ "$STAGE" = prof ]; then
  rm -rf $OUT/prof
  timeout -k 10 ${PROF_TIMEOUT:-400} rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python3 bench.py --full --steps 50 --warmup 10 --no-cpu --no-extra > $OUT/prof.log 2>&1
  ok_or_stop $? rocprof
  find $OUT/prof -name '*kernel_stats*' | head -3
fi
exit 0
