#!/bin/bash
# rocprofv3 kernel trace of the bench command, serial (MART_OVERLAP_WGRAD=0) and as shipped; summaries -> $OUT_DIR/
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT_DIR=${OUT_DIR:-out}; mkdir -p "$OUT_DIR"    # logs and summaries (OUT_DIR=... to put them elsewhere)
for mode in serial overlap; do
  if [ $mode = serial ]; then export MART_OVERLAP_WGRAD=0 MART_TWO_STREAM=0; else export MART_OVERLAP_WGRAD=1 MART_TWO_STREAM=1; fi
  rm -rf $OUT_DIR/prof_tmp
  timeout 600 rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof_tmp -- python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > $OUT_DIR/prof_$mode.log 2>&1
  DB=$(find $OUT_DIR/prof_tmp -name "*.db" | head -1)
  python tools/rocpd_stats.py $DB > $OUT_DIR/r01_bench_kernel_stats_v17_$mode.csv
  tail -1 $OUT_DIR/prof_$mode.log | cut -c1-300
  rm -rf $OUT_DIR/prof_tmp
done
unset MART_OVERLAP_WGRAD MART_TWO_STREAM
timeout 400 python bench.py --full 2>&1 | tail -1 > $OUT_DIR/bench_v17.json
