#!/bin/bash
# One GPU-box evidence round (round 4): bench (headline + sub-blocks + CPU baselines), rocprofv3 kernel statistics of the
# headline command (two-stream and one-stream) and of the Painter-forward block, the whole-step HBM budget (PMC passes + call
# log) and the SPADE PMC passes.  Outputs under $OUT (default out/) ; summaries are copied to profiles/ by tools (kstats, budget).
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-r04}
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -2) > $OUT/smoke.log 2>&1
(timeout 1700 python bench.py --full --conv-table $OUT/conv_table_$TAG.txt 2>&1 | tail -1) > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o $TAG -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --sub-steps 0 --mfma-table-steps 0 2>&1 | tail -1) > $OUT/rocprof_$TAG.log 2>&1
(CGAN_OVERLAP=0 timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_serial -o ${TAG}_serial -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --sub-steps 0 --mfma-table-steps 0 2>&1 | tail -1) > $OUT/rocprof_${TAG}_serial.log 2>&1
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_painter -o ${TAG}_painter -- python bench.py --only painter --steps 7 --warmup 2 2>&1 | tail -1) > $OUT/rocprof_${TAG}_painter.log 2>&1
rm -f $OUT/prof_$TAG/*kernel_trace.csv $OUT/prof_${TAG}_painter/*kernel_trace.csv $OUT/prof_${TAG}_serial/*kernel_trace.csv
bash tools/gpu_budget.sh $TAG > /dev/null 2>&1
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_${TAG}p_$ctr
  (timeout 600 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $OUT/pmc_${TAG}p_$ctr -o ${TAG}p -- \
     python bench.py --only painter --steps 1 --warmup 1 2>&1 | tail -1 | cut -c1-200) > $OUT/pmc_${TAG}p_$ctr.log 2>&1
  rm -f $OUT/pmc_${TAG}p_$ctr/*kernel_trace.csv
done
cat $OUT/smoke.log; cut -c1-600 $OUT/bench_$TAG.json; ls $OUT/prof_$TAG $OUT/prof_${TAG}_serial $OUT/prof_${TAG}_painter $OUT/pmc_${TAG}p_FETCH_SIZE
