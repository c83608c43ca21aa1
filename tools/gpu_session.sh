#!/bin/bash
# One GPU session on the box: new/changed GPU tests first, then the whole GPU suite, smoke, and a
# short bench line.  Usage: bash tools/gpu_session.sh <outdir> [pytest -k expression for the first step]
OUT=${1:-gpurun_out/session}
K=${2:-}
mkdir -p $OUT
export TMPDIR=/tmp
if [ -n "$K" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -k "$K" > $OUT/pytest_first.log 2>&1
  rc=$?; tail -5 $OUT/pytest_first.log; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -3 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -5 $OUT/smoke.log; exit 1; }
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err || { tail -5 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
