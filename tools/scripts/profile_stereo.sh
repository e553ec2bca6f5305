: ${GRAFT_REPO_ROOT:?run on the GPU box (gpurun exports it): an empty root would turn cd / rm -rf below into operations on /}
set -e
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"             # where the results land
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_2ch -- python $R/bench.py --full --no-cpu --no-configs --channels 2 --steps 100 --warmup 10 > $OUT/bench_2ch.json 2>/dev/null
cd $R
find $OUT/prof_2ch -name "*kernel_stats.csv" -exec cp {} $OUT/kernel_stats_2ch.csv \;
rm -rf $OUT/prof_2ch
head -8 $OUT/kernel_stats_2ch.csv | cut -c1-170
python3 -c "
import json
d=json.loads(open('$OUT/bench_2ch.json').read().strip().split('\n')[-1]); print(d['value'], d['ms_per_step'], d['kernel_ms'])"
