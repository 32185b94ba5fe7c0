#!/bin/bash
# GPU parity tests, then the full bench line with its per-kernel breakdown (no rocprof).  Output folder: $OUT (default tool_out/).
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/tool_out}
cd "$R"; mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== pytest gpu"; timeout 1500 python -m pytest tests -x -q -m gpu 2>&1 | tail -8
echo "== bench" ; timeout 900 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --detail "$OUT/bench_detail_train_n1.json" 2>&1 | tail -1 > "$OUT/bench_line.json"
python - "$OUT/bench_detail_train_n1.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print('ms_per_step', d['ms_per_step'], 'value', d['value'])
for k in d['roofline']['all_kernel_families']:
    print(f"  {k['kernel'][:50]:50s} {k['launches_per_step']:6.1f}/step avg {k['avg_us']:8.1f} us  {k['ms_per_step']:6.3f} ms/step  {k['achieved']:8.1f} {k['unit']}")
PY
