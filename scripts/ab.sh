#!/bin/bash
# usage (GPU box): scripts/r4_ab.sh lib1.so lib2.so ...   -- C3 bench per library: serial kernel table + pipelined views/s
R=$(cd "$(dirname "$0")/.." && pwd)
O=${TEXGS_OUT:-$R/out}
cd "$R"
mkdir -p "$O"
for V in "$@"; do
for MODE in "--streams 1" ""; do
TEXGS_LIB=$R/texture-gs_amd/$V timeout 400 python bench.py --full --no-cpu-baseline --steps 8 --warmup 3 $MODE 2> $O/ab_err.log | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); print('$V', '$MODE', d['value'], {k:round(v['avg_us']) for k,v in d['kernels'].items()}, (d.get('reference_call_pattern') or {}).get('views_per_s'))
"
done
done
tail -3 $O/ab_err.log
