# 8 ch x 60 s round trips at the ( window hop dft ) shapes in $SHAPES (";"-separated), optional $VARIANT for --kernel-variant; result lines in $OUT/shapes_$TAG.txt
: ${SHAPES:?}
TAG=${TAG:-run}
OUT=${OUT:-bench_out}             # where the results land
cd "$(dirname "$0")/../.." && mkdir -p "$OUT" && : > $OUT/shapes_$TAG.txt
IFS=';' read -ra LIST <<< "$SHAPES"
for cfg in "${LIST[@]}"; do set -- $cfg
  timeout -k 10 180 python bench.py --full --window $1 --hop $2 --dft $3 --no-cpu --no-configs --steps ${STEPS:-10} --warmup 3 ${VARIANT:+--kernel-variant $VARIANT} > $OUT/bench_shape_$1_$2_$3.json 2> $OUT/bench_shape_$1_$2_$3.err || { echo "$1 $2 $3 FAILED" >> $OUT/shapes_$TAG.txt; tail -3 $OUT/bench_shape_$1_$2_$3.err >> $OUT/shapes_$TAG.txt; continue; }
  python -c "
import json
d=json.loads(open('$OUT/bench_shape_$1_$2_$3.json').read().strip().splitlines()[-1]); print($1, $2, $3, d['ms_per_step'], round(d['value']/1e6,2), 'M frames/s', d['roundtrip_hbm']['frac_of_8TBs'], {k: v for k, v in d.get('kernel_ms', {}).items() if k != 'note'})" >> $OUT/shapes_$TAG.txt
done
cat $OUT/shapes_$TAG.txt
