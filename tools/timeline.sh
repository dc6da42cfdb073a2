#!/bin/bash
# tools/timeline.sh TAG [env...] -- on the GPU box: kernel trace of the default (four-stream) C2 bench and of the recorded batch-32 step, summarised by tools/timeline_gaps.py
set -e
TAG=$1
R=$PWD
OUT_DIR=${OUT_DIR:-results}          # summaries and logs go here (relative to the repository root)
mkdir -p $OUT_DIR
export TMPDIR=/tmp
cd /tmp
rocprofv3 --kernel-trace --output-format csv -d $R/$OUT_DIR/${TAG}_tl -- python3 $R/bench.py --full --no-cpu-baseline --no-extras --alt-precision "" --steps 6 --warmup 3 > $R/$OUT_DIR/${TAG}_tl_bench.json 2> $R/$OUT_DIR/${TAG}_tl.err
cd $R
python tools/timeline_gaps.py $(find $OUT_DIR/${TAG}_tl -name "*kernel_trace.csv" | head -1) 0.5 > $OUT_DIR/${TAG}_timeline_c2.txt
rm -rf $OUT_DIR/${TAG}_tl
cd /tmp
rocprofv3 --kernel-trace --output-format csv -d $R/$OUT_DIR/${TAG}_tl32 -- python3 $R/tools/recorded_profile.py train 32 > $R/$OUT_DIR/${TAG}_tl32.txt 2> $R/$OUT_DIR/${TAG}_tl32.err
cd $R
python tools/timeline_gaps.py $(find $OUT_DIR/${TAG}_tl32 -name "*kernel_trace.csv" | head -1) 0.6 > $OUT_DIR/${TAG}_timeline_b32_recorded.txt
rm -rf $OUT_DIR/${TAG}_tl32
cat $OUT_DIR/${TAG}_timeline_c2.txt $OUT_DIR/${TAG}_timeline_b32_recorded.txt
