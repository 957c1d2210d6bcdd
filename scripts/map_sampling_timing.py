"""Cost of the weighted map-pool sampling and the per-map episode statistics (mgx_set_pool_sampling, mgx_set_map_stats):
wall-clock mean step of MettaGridBatchedEnv at the benchmark shape — rung-3 rules (32 x 32, 16 agents), 65 536 envs, a 16-map
device pool with on-device auto-reset, max_steps = 128, desync=True, unchecked actions — with the rotation rule, with sampling
(uniform weights) and with sampling plus map statistics, three wrappers in one process.  Episode statistics are on in all
three.  After a warm-up round the variants alternate round by round (interleave what you compare, report the spread): every
round times `steps` steps of each variant in turn; per variant the median over the rounds is reported with min / max and the
coefficient of variation.  The yardstick is the rotation variant of the same process.  With desync about E / max_steps envs
finish per step, so the draw kernel and the table kernel walk a list of about 512 entries.  Prints one JSON line.
Usage (GPU box): python scripts/map_sampling_timing.py [envs] [steps] [rounds]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.envs import MettaGridBatchedEnv  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5

spec = presets.rung3_spec()
spec.max_steps = 128
prog = compile_spec(spec, 32, 32, max_objects=192)
A = prog.num_agents
pool = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(16))
VARIANTS = {"rotation": {}, "sampling": {"map_weights": "uniform", "map_sample_seed": 5},
            "sampling_stats": {"map_weights": "uniform", "map_sample_seed": 5, "map_stats": True}}
envs = {}
for name, kw in VARIANTS.items():
    envs[name] = MettaGridBatchedEnv(prog, E, map_pool=pool, pool_stride=7, desync=True, validate_actions=False, seed=1, **kw)
    envs[name].reset()
gen = torch.Generator(device="cuda").manual_seed(3)
acts = torch.randint(0, int(envs["rotation"].transport_action_n), (8, E * A), dtype=torch.int32, device="cuda", generator=gen)


def run(env, n: int) -> dict:
    last = {}
    for t in range(n):
        *_, infos = env.step(acts[t % 8])
        last = infos or last
    return last


ms = {k: [] for k in VARIANTS}
last = {}
for r in range(rounds + 1):   # round 0 is the warm-up: played (through the first, desynchronised episodes), not reported
    for name, env in envs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[name] = run(env, steps)
        torch.cuda.synchronize()
        if r:
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
out = {"envs": E, "steps": steps, "rounds": rounds, "maps": int(pool.shape[0]),
       "episodes_in_last_window": {k: int(v.get("episodes", 0)) for k, v in last.items()},
       "map_episodes_in_last_window": [m["episodes"] for m in last["sampling_stats"].get("per_map", [])]}
for name in VARIANTS:
    a = np.asarray(ms[name])
    out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                 "cv_pct": round(float(a.std() / a.mean() * 100), 2), "ms_rounds": [round(float(x), 4) for x in a]}
out["rotation_range_ms"] = round(out["rotation"]["ms_max"] - out["rotation"]["ms_min"], 4)
for name in ("sampling", "sampling_stats"):
    out[f"{name}_minus_rotation_ms_median"] = round(out[name]["ms_median"] - out["rotation"]["ms_median"], 4)
print(json.dumps(out), flush=True)
for env in envs.values():
    env.close()
