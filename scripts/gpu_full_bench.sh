# The full bench.py run (--full) end to end, timed, with the fields of its line printed (GPU box).
# Usage: bash scripts/gpu_full_bench.sh <output dir>
OUT="${1:?usage: bash scripts/gpu_full_bench.sh <output dir>}"
mkdir -p "$OUT"
( time timeout -k 10 900 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err" ) 2> "$OUT/time.txt" || { tail -5 "$OUT/bench_full.err"; exit 1; }
tail -3 "$OUT/time.txt"
python - "$OUT/bench_full.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
for k in ('metric','value','unit','ms_per_step','n_gpus','steps','vs_baseline','dtype','scaling','variants','kernels_ms','roofline','cpu_baseline','long_run','generic','run_time_specialisation','env_wrapper'):
    print(k, d.get(k))
print([k for k in d.keys()])
PY
