#!/bin/bash
# full GPU suite + the full bench line (CPU baseline and discopt included):  bash tools/gpu_full.sh OUT_DIR
out=${1:?usage: bash tools/gpu_full.sh OUT_DIR}
mkdir -p "$out"
timeout 1800 python -m pytest tests -m gpu -x -q > "$out/full_pytest.log" 2>&1; echo "pytest rc=$?"; grep -E "passed|failed|error" "$out/full_pytest.log" | tail -3
timeout 900 python bench.py --full --steps 5 --warmup 2 > "$out/full_bench.json" 2> "$out/full_bench.err"; echo "bench rc=$?"; tail -c 400 "$out/full_bench.err"
python - "$out" <<'PY'
import json, os, sys
d = json.load(open(os.path.join(sys.argv[1], "full_bench.json")))
print("value %.5g  kernel %.2f ms  %s  discopt %.1f it/s  cpu %.0f" % (d["value"], d["roofline"]["kernel_avg_ms"], d["config"]["kernel_variant"], d["discopt"]["iters_per_s"], d["cpu_baseline"]["value"]))
PY
