#!/bin/bash
# usage (GPU box): tools/ab_env.sh "ENV=1 ..." "ENV2=..." ...  -- bench.py --full (cfg2 + also) once per environment setting ("" = default)
# logs: $BENCH_LOGS (default bench_out/)
out=${BENCH_LOGS:-bench_out}
mkdir -p $out
i=0
for e in "$@"; do
  i=$((i+1))
  env $e timeout 600 python bench.py --full --verbose --no-cpu-baseline --steps 100 --windows 11 > $out/abenv_$i.log 2>&1 || tail -5 $out/abenv_$i.log
  python tools/bench_compact.py $out/abenv_$i.log "[${e:-default}]"
done
