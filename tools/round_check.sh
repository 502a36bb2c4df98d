#!/usr/bin/env bash
# Round-end check on a GPU machine: full GPU test suite, smoke(), the full bench line.
#   tools/round_check.sh <tag> [out_dir]  -> <out_dir>/pytest_<tag>.log, <out_dir>/bench_<tag>.json
set -o pipefail
TAG=${1:-chk}
OUT=${2:-check_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 250 --timeout-method thread > "$OUT/pytest_$TAG.log" 2>&1
rc=$?; tail -2 "$OUT/pytest_$TAG.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 || exit 1
timeout -k 10 500 python bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err" || { tail -5 "$OUT/bench_$TAG.err"; exit 1; }
python - "$OUT/bench_$TAG.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(round(d["value"]), round(d["valu_roofline"]["frac"], 3), "msm", round(d["msm"]["value"] / 1e6, 1),
      "pip", round(d["msm"]["pippenger"]["value"] / 1e6, 1), "ipa", round(d["ipa"]["value"]), "prove",
      round(d["prove"]["value"]), "shard", round(d["sharded_2p16"]["value"]), "host", round(d["host_api"]["value"]),
      "cpu", round(d["cpu_baseline"]["value"], 1))
PY
