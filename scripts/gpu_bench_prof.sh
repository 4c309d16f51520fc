#!/bin/bash
# bench at the default workload + rocprofv3 kernel stats of the same command
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/bench_out}          # where the results land (set OUT to collect them elsewhere)
cd "$ROOT"; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
TAG=${1:-x}
python bench.py --full --steps 10 --warmup 2 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
tail -2 $OUT/bench_$TAG.err; cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $ROOT/bench.py --full --steps 10 --warmup 2 --cpu-baseline off > $OUT/prof_${TAG}_stdout.txt 2>&1
grep '^{' $OUT/prof_${TAG}_stdout.txt | cut -c1-300
head -14 $OUT/prof_$TAG/*/*_kernel_stats.csv | cut -c1-160
cp $OUT/prof_$TAG/*/*_kernel_stats.csv $OUT/kernel_stats_$TAG.csv
