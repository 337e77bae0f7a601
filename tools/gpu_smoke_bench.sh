#!/bin/bash
# smoke() on cuda:0, then the full bench line (bench.py --full: every leg).
# Usage: bash tools/gpu_smoke_bench.sh TAG  -> $M2DEC_AMD_OUT/bench_TAG.json (default bench_out/)
set -o pipefail
TAG=${1:-final}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${M2DEC_AMD_OUT:-bench_out}
cd $R && mkdir -p $O
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" || exit $?
timeout -k 10 600 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err || exit $?
python3 - $O/bench_$TAG.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
s = d["gpu_recon_streams"]
print("value", d["value"], "traffic", d["roofline"]["traffic"], "gpu_recon", d["gpu_recon"]["value"],
      "streams", s["value"], s["roofline"]["traffic"], "c5", d["end_to_end_c5"]["value"])
PY
