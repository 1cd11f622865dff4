#!/bin/bash
# the round-end sequence on this tree: every -m gpu test, smoke(), the whole bench line (--full)
# usage (GPU box): bash tools_dev/gpu_final.sh [tag]   (logs under $OUT_ROOT/<tag>, default out/<tag>)
set -o pipefail
T=${1:-final}
cd "$(dirname "$0")/.." || exit 9
OUT=${OUT_ROOT:-out}/$T
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests/ -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo "pytest failed"; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -1 $OUT/gpu_tests.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail $OUT/smoke.log; exit 2; }
tail -1 $OUT/smoke.log
timeout -k 10 900 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail $OUT/bench.err; exit 3; }
python3 -c "import json;d=json.load(open('$OUT/bench.json'));print(d['value'],d['ms_per_step'],d['parity_all_steps'],{k:(v.get('value') if isinstance(v,dict) else None) for k,v in d.items() if isinstance(v,dict) and 'value' in v})"
