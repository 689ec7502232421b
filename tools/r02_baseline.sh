#!/bin/bash
# Round-2 baseline: cold-cache bench line with extras (--full), then SQ/TCP/TCC counter passes in cold mode.
# Usage: tools/r02_baseline.sh OUTDIR (raw output)
set -o pipefail
cd "$(dirname "$0")/.."
OUT="$(mkdir -p "${1:?usage: tools/r02_baseline.sh OUTDIR}" && cd "$1" && pwd)" || exit 1
export OUT
export TMPDIR=/tmp
timeout -k 10 500 python bench.py --full --no-cpu > $OUT/r02_bench0.json 2> $OUT/r02_bench0.err || { tail -20 $OUT/r02_bench0.err; exit 1; }
python - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ['OUT'], 'r02_bench0.json')))
print('headline', round(d['value'],1), 'ms', round(d['ms_per_step'],4), 'frac', round(d['roofline']['frac'],4), d['roofline']['device_ms_per_step_blocks'])
for k,v in d['extra'].items():
    if isinstance(v,dict): print(k, round(v['device_ms_per_step'],4), round(v['Mpix_edges_per_s'],1), v.get('roofline_frac'))
    else: print(k, v)
PY
BENCH_ARGS="--no-extra" bash tools/run_pmc_bench.sh > $OUT/r02_pmc_cold.txt 2>&1
cat $OUT/r02_pmc_cold.txt
