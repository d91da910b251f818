#!/bin/bash
# Kernel trace (rocprofv3 --kernel-trace --stats) of the whole benchmark, every leg (bench.py --full).
#   scripts/gpu_trace.sh <tag> [out-dir]     (default out-dir: out/)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
R=${1:-r04}
OUT=${2:-out}/trace_$R
mkdir -p $OUT
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT -o $R --output-format csv -- python3 -u bench.py --full \
  > $OUT/bench.json 2> $OUT/bench.err
rc=$?
echo "trace rc=$rc"
find $OUT -name "*stats*"
exit $rc
