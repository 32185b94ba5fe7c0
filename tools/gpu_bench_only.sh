#!/bin/bash
# The full bench line with its per-kernel-family table, then rocprofv3 --kernel-trace --stats of the same command.
# Output folder: $OUT (default tool_out/).
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/tool_out}
cd "$R"; mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== bench" ; timeout 900 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --detail "$OUT/bench_detail_train_n1.json" > /dev/null 2>&1
python - "$OUT/bench_detail_train_n1.json" <<'PY'
import sys, json
d = json.load(open(sys.argv[1]))
print('ms_per_step', d['ms_per_step'], 'value', d['value'])
for k in d['roofline']['all_kernel_families']:
    print(f"  {k['kernel'][:50]:50s} {k['launches_per_step']:6.1f}/step avg {k['avg_us']:8.1f} us  {k['ms_per_step']:6.3f} ms/step  {k['achieved']:8.1f} {k['unit']}")
PY
echo "== rocprof" ; (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --no-cpu-baseline --detail "$OUT/bench_detail_prof.json" > "$OUT/rocprof.log" 2>&1)
f=$(find "$OUT/prof" -name "*kernel_stats.csv" | sort | tail -1); echo "stats: $f"; python - "$f" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
steps = max(int(r["Calls"]) for r in rows if "grid_to_ndhwc8" in r["Name"])    # one launch per step (priming + warm-up + timed + replay)
print(f"total GPU ms per step ({steps} steps):", tot / steps / 1e6)
for r in rows[:28]:
    print(f'{r["Name"][:90]:90s} calls/step {int(r["Calls"])/steps:6.1f} avg {float(r["AverageNs"])/1e3:8.1f} us  {float(r["TotalDurationNs"])/steps/1e6:6.3f} ms/step')
PY
