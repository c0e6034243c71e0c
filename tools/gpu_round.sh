#!/bin/bash
# One GPU-box round: parity tests, smoke, bench (headline + sub-blocks + CPU baselines), and the rocprofv3 kernel statistics
# of the headline command and of the Painter-forward sub-block.  Outputs under $OUT (default out/) ; summaries are copied to
# profiles/ by hand (tools/kstats.py, tools/summarize_trace.py).
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-r03}
if [ -z "$SKIP_TESTS" ]; then
(timeout 2400 python -m pytest tests -m gpu -q --durations=8 2>&1 | tail -40) > $OUT/pytest_gpu.log 2>&1
fi
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -3) > $OUT/smoke.log 2>&1
(timeout 1500 python bench.py --full 2>&1 | tail -2) > $OUT/bench.log 2>&1
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o $TAG -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --sub-steps 0 2>&1 | tail -2) > $OUT/rocprof.log 2>&1
# the same command with both branches on one stream: kernel durations without a concurrent kernel next to them
(CGAN_OVERLAP=0 timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_serial -o ${TAG}_serial -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --sub-steps 0 2>&1 | tail -2) > $OUT/rocprof_serial.log 2>&1
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_painter -o ${TAG}_painter -- python bench.py --only painter --steps 7 --warmup 2 2>&1 | tail -2) > $OUT/rocprof_painter.log 2>&1
for f in pytest_gpu smoke bench rocprof rocprof_serial rocprof_painter; do echo "=== $f"; tail -n 12 $OUT/$f.log | cut -c1-3000; done
ls $OUT/prof_$TAG/* $OUT/prof_${TAG}_painter/* 2>/dev/null | head
