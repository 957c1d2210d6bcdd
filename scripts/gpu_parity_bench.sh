# Bounded small test first, then the parity files, then a rung-3 and a rung-4 bench line (GPU box).
# Usage: bash scripts/gpu_parity_bench.sh <output dir>
set -e
OUT="${1:?usage: bash scripts/gpu_parity_bench.sh <output dir>}"
mkdir -p "$OUT"
timeout -k 10 150 python -m pytest tests/test_gpu_golden.py -x -q -k "rung3 or rung2 or torture" > "$OUT/small.log" 2>&1 || { tail -30 "$OUT/small.log"; exit 1; }
tail -2 "$OUT/small.log"
timeout -k 10 900 python -m pytest tests/test_gpu_act.py tests/test_gpu_golden.py tests/test_gpu_parity.py tests/test_gpu_scale.py tests/test_gpu_long_horizon.py tests/test_gpu_gen.py tests/test_gpu_episode_stats.py tests/test_gpu_envs.py -x -q > "$OUT/tests.log" 2>&1 || { tail -40 "$OUT/tests.log"; exit 1; }
tail -3 "$OUT/tests.log"
timeout -k 10 200 python bench.py --full --steps 200 --warmup 20 --no-cpu --no-extras > "$OUT/b3.json" 2> "$OUT/b3.err"
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print('rung3', round(d['value']/1e6,1), d['ms_per_step'], d['kernels_ms'], d['variants'])" "$OUT/b3.json"
timeout -k 10 300 python bench.py --full --rung 4 --steps 60 --warmup 10 --no-cpu --no-extras > "$OUT/b4.json" 2> "$OUT/b4.err"
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print('rung4', round(d['value']/1e6,1), d['ms_per_step'], d['kernels_ms'], d['variants'])" "$OUT/b4.json"
