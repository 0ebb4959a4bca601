#!/bin/bash
# usage (GPU box): tools/ab.sh libA.so libB.so ...   -- bench.py --full (cfg2 + also) once per library, compact lines
# logs: $BENCH_LOGS (default bench_out/)
out=${BENCH_LOGS:-bench_out}
mkdir -p $out
for lib in "$@"; do
  tag=$(basename $lib .so)
  CMAX_LIB=$lib timeout 600 python bench.py --full --verbose --no-cpu-baseline --no-pmc --steps 100 --windows 11 > $out/ab_$tag.log 2>&1 || tail -5 $out/ab_$tag.log
  python tools/bench_compact.py $out/ab_$tag.log "[$tag]"
done
