#!/bin/bash
# round 5, call 10: the driver-style bench line (profiles/r05_bench_default.json); usage: bash c10.sh OUTDIR
set -e
D=${1:?usage: c10.sh OUTDIR}
mkdir -p "$D"
timeout -k 10 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$D/bench_default.json" 2> "$D/bench_default.err" || { tail -20 "$D/bench_default.err"; exit 1; }
python - "$D/bench_default.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print('value', d['value'], 'runs', d['value_runs'])
print('roofline', d['roofline']['frac'], d['roofline']['second_kernel']['frac'], d['roofline']['traffic'], d['roofline']['traffic_note'][:50])
print('C', d['units']['C']['achieved'], d['units']['C']['frac'], 'B', d['units']['B']['value'], d['units']['B']['frac'], d['units']['B']['single_level']['frac'])
for k,v in d['configs'].items(): print(k, v['value'], v['parity']['ok'], v.get('hbm'))
print('c4', d['config4']['value'], d['config4']['parity']['ok'])
print('A', d['units']['A']['ceiling_shared_datapath_units_per_s'])
print('cpu', d['cpu_baseline']['value'], d['sate_rel_err'])
PY
