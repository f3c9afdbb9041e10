#!/bin/bash
# rocprofv3 kernel statistics of the two train legs, one trace per mode (profiles/rNN/bench_kernel_stats_{full,lora}.csv).
# Usage: bash scripts/prof_train.sh [output directory, default prof_out]
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
O=${1:-prof_out}
mkdir -p $O
export ECGB_BENCH_WORKERS=1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_full -o full -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-c1 --no-c5 --no-lora-leg --no-extras --train-steps 3 > $O/prof_full.json 2> $O/prof_full.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_lora -o lora -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-c1 --no-c5 --lora --no-extras --train-steps 3 > $O/prof_lora.json 2> $O/prof_lora.err
find $O/prof_full $O/prof_lora -name "*kernel_stats.csv" | head
for f in $(find $O/prof_full $O/prof_lora -name "*kernel_stats.csv"); do echo == $f; head -25 $f | cut -c1-200; done
# keep only the stats (the traces are large)
find $O/prof_full $O/prof_lora -type f ! -name "*stats.csv" -delete
