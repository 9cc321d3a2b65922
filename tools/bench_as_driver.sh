#!/bin/bash
# the full bench line (python bench.py --full), its wall time, and the fields a reader looks at first:  bash tools/bench_as_driver.sh [DIR]
# (the line and its stderr are kept in DIR, by default a new temporary directory)
cd "$(dirname "$0")/.."; OUT=${1:-$(mktemp -d)}; mkdir -p "$OUT"
SECONDS=0
python3 bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"
echo "rc $? wall ${SECONDS} s, output in $OUT"
python3 - "$OUT" <<'PY'
import json, sys
d = json.loads([l for l in open(f"{sys.argv[1]}/bench_final.json") if l.startswith("{")][-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["traffic"], d["cpu_baseline"])
print(d["cfg3"]["value"], d["cfg3"]["roofline"]["traffic"], d["cfg4_n1"]["value"], d["cfg4_n1"]["roofline"]["frac"], d["cfg5"]["guided_ms_per_frame"], d["cfg5"]["both_ms_per_frame"])
PY
