#!/bin/bash
# config [4] quick look: the bench line's phases and the rocprofv3 kernel stats of the same command (GPU box, from the repo root;
# outputs land in $OUT, default out/)
R="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "${OUT:=$R/out}" && OUT="$(cd "$OUT" && pwd)" && export OUT
python3 "$R/bench.py" --full --config envs --steps 100 2>/dev/null > "$OUT/envs_line.json"
python3 - "$OUT/envs_line.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print("value", d["value"], "closed_loop", (d.get("closed_loop") or {}).get("value"))
for k, v in d.items():
    if isinstance(v, dict) and any(x.endswith("_us") for x in v): print(k, v)
PY
cd /tmp && export TMPDIR=/tmp
rm -rf "$OUT/prof_envs"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_envs" -o envs -- python3 "$R/bench.py" --full --config envs --steps 30 --warmup 5 --no-closed-loop > /dev/null 2>&1
cd "$R"
find "$OUT"/prof_envs -name "*kernel_stats.csv" -exec cp {} "$OUT"/envs_kernel_stats.csv \;
rm -rf "$OUT"/prof_envs
python3 - <<'PY'
import csv, os
rows = list(csv.DictReader(open(os.environ["OUT"] + "/envs_kernel_stats.csv")))
n = max(int(r["Calls"]) for r in rows if "noise_gemm" in r["Name"])
for r in rows[:14]:
    print(r["Name"][:44].ljust(46), r["Calls"].rjust(6), "%8.2f us" % (float(r["AverageNs"]) / 1e3), "%7.1f us/step" % (float(r["TotalDurationNs"]) / 1e3 / n), r["Percentage"])
PY
