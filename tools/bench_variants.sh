#!/bin/bash
# tools/bench_variants.sh <dir/prefix> "VAR=val VAR2=val" "..." : one bench.py --full line per environment variant -> <dir/prefix>_v<i>.json
pre=$1; shift
mkdir -p "$(dirname "$pre")"
i=0
for v in "$@"; do
  i=$((i+1))
  env $v timeout 120 python bench.py --full --no-cpu-baseline --repeats 3 > ${pre}_v$i.json 2> ${pre}_v$i.err
  python - <<P
import json
try:
    d=json.loads(open("${pre}_v$i.json").read().strip().splitlines()[-1])
    print("$v".ljust(44), d["ms_per_step"], {k: d["phases_us"][k] for k in ("rec_fwd","output","rec_bwd","wgrad","scatter","update")})
except Exception as e:
    print("$v", "FAILED", e); print(open("${pre}_v$i.err").read()[-600:])
P
done
