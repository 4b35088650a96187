#!/bin/bash
# idle-gap analysis of the shipped (three-stream) schedule: rocprofv3 kernel trace of a short bench run -> tools/rocpd_stats.py
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT_DIR=${OUT_DIR:-out}; mkdir -p "$OUT_DIR"    # logs and summaries (OUT_DIR=... to put them elsewhere)
rm -rf $OUT_DIR/prof_tmp
timeout 600 rocprofv3 --kernel-trace -d $OUT_DIR/prof_tmp -- python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-kernel-timing > $OUT_DIR/gaps.log 2>&1
DB=$(find $OUT_DIR/prof_tmp -name "*.db" | head -1)
python tools/rocpd_stats.py $DB | grep "^#"
rm -rf $OUT_DIR/prof_tmp
