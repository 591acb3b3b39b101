#!/bin/bash
# full -m gpu suite, then the full bench line (--full: legs, rank, CPU baselines); logs and the line go to OUT_DIR
OUT=$(realpath -m "${1:?usage: bash tools/run_suite.sh OUT_DIR}")
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout 2400 python -m pytest tests -x -q -m gpu --durations=12 > "$OUT/suite.log" 2>&1
echo "pytest rc=$?" >> "$OUT/suite.log"
tail -30 "$OUT/suite.log"
timeout 900 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
echo "bench rc=$?"
tail -3 "$OUT/bench.err"
BENCH_JSON="$OUT/bench.json" python - <<'PY'
import json, os
j=json.load(open(os.environ["BENCH_JSON"]))
print({k:j[k] for k in ("value","ms_per_step")}, j["roofline"], j.get("cpu_baseline"))
print(j["config"].get("form"), j["train_stats"])
for n,l in j.get("legs",{}).items(): print(n, {k:l.get(k) for k in ("value","ms_per_step","error")}, l.get("roofline",{}).get("frac"), l.get("roofline",{}).get("kernel"))
print(j["rank"]["ms"], j["rank"]["roofline"]["frac"])
PY
