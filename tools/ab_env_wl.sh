#!/bin/bash
# usage (GPU box): tools/ab_env_wl.sh <workload> "ENV=1 ..." "ENV2=..." ...  -- one workload, once per environment setting ("" = default)
# logs: $BENCH_LOGS (default bench_out/)
wl=$1; shift
out=${BENCH_LOGS:-bench_out}
mkdir -p $out
i=0
for e in "$@"; do
  i=$((i+1))
  env $e timeout 600 python bench.py --full --verbose --no-cpu-baseline --no-also --workload $wl --steps 100 --windows 11 > $out/abenvwl_$i.log 2>&1 || tail -5 $out/abenvwl_$i.log
  python tools/bench_compact.py $out/abenvwl_$i.log "[${e:-default}]"
done
