#!/bin/bash
# A/B of the flow-table load factor (rxg_tune_flow_load) on cfg4, interleaved
# bench processes on one box: --flow-load N = exact-key tables at load <= 2^-N
# (--full: the oracle parity sample of every run is printed beside its times)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for i in 1 2; do
  for fl in ${FLS:-1 2}; do
    timeout -k 10 200 python bench.py --full --workload cfg4 --no-cpu --no-cfg1 --no-tx --steps 20 --flow-load $fl > "$OUT/b_fl${fl}_$i.log" 2>&1 || exit 1
    python3 -c "
import json
for l in open('$OUT/b_fl${fl}_$i.log'):
    if l.startswith('{'): d=json.loads(l); print('flow_load', $fl, 'rep', $i, 'ms_per_step', d['ms_per_step'], 'parity', d['parity']['mismatches'])
"
  done
done
echo ALLDONE
