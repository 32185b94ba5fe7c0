#!/bin/bash
# One GPU-box session: tests, smoke, stage times, the full bench line, rocprof.  Everything lands in $OUT (default tool_out/).
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/tool_out}
cd "$R"; mkdir -p "$OUT"
export TMPDIR=/tmp
echo "== pytest -m gpu" ; timeout 1200 python -m pytest tests -q -m gpu --timeout=900 2>&1 | tail -15 | tee "$OUT/pytest_gpu.log"
echo "== smoke" ; timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 | tee "$OUT/smoke.log"
echo "== stages"; timeout 600 python tools/stage_bench.py 2>&1 | grep -v amdgpu.ids | tee "$OUT/stage_bench.log"
echo "== bench" ; timeout 900 python bench.py --full --steps 20 --warmup 5 --detail "$OUT/bench_detail_train_n1.json" 2>&1 | tail -2 | tee "$OUT/bench.log"
echo "== rocprof" ; (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --no-cpu-baseline --detail "$OUT/bench_detail_prof.json" > "$OUT/rocprof.log" 2>&1)
tail -2 "$OUT/rocprof.log" | cut -c1-300
f=$(find "$OUT/prof" -name "*kernel_stats.csv" | sort | tail -1); echo "stats: $f"; head -22 "$f" | cut -c1-160
