#!/bin/bash
# usage: tools/ab_env.sh VAR v1 v2 ... : short bench per value of an environment variable, prints ms/pass + per-class GEMM medians
var=$1; shift
for v in "$@"; do
  env $var=$v timeout -k 10 200 python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --streams 0 2>/dev/null |
    python -c 'import json, sys; d = json.loads(sys.stdin.read().strip().splitlines()[-1]); print(sys.argv[1], d["ms_per_step"], d["roofline"]["all_ops_us"])' "$var=$v"
done
