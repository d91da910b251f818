#!/bin/bash
# round record: full GPU suite (verbose), smoke(), then the whole bench line (bench.py --full) twice
#   scripts/gpu_record.sh <tag> [out-dir]     (default out-dir: out/)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
R=${1:-record}
OUT=${2:-out}/$R
mkdir -p $OUT
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread \
  > $OUT/gpu_tests.log 2>&1 || { echo "tests rc=$?"; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 \
  || { echo "smoke rc=$?"; tail -30 $OUT/smoke.log; exit 1; }
tail -2 $OUT/smoke.log
for k in a b; do
  timeout -k 10 400 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_$k.json 2> $OUT/bench_$k.err \
    || { echo "bench rc=$?"; tail -30 $OUT/bench_$k.err; exit 1; }
  cut -c1-300 $OUT/bench_$k.json
done
