cd "$(dirname "$0")/.."; out=${1:?usage: tools/gpu_dead_out.sh OUTPUT_DIR}
mkdir -p "$out"
timeout 900 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "unread_irreps or structural_zero or full_size or default_irreps or refresh" > "$out/tests.log" 2>&1
echo "tests exit $?" >> "$out/tests.log"
tail -5 "$out/tests.log"
timeout 600 python bench.py --full > "$out/bench.json" 2> "$out/bench.err"
echo "bench exit $?"
python - "$out/bench.json" <<'PY'
import json, sys
r = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(r["value"], r["ms_per_step"], r["roofline"]["frac"], r["roofline"]["frac_full_program_launches"], r["roofline"]["frac_without_structural_zero_flops"])
print(r["roofline"]["launch_ms_by_position_in_step"], r["roofline"]["nonzero_flop_share_by_position"])
print({k: v for k, v in r.items() if "accuracy" in k})
PY
