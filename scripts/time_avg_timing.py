"""Cost of the time-averaged game stats (mgx_set_time_averages): event-timed mean step of the rung-3 benchmark shape (32 x 32, 16
agents) with the feature off and on, in one process on one engine.  Episode statistics are on in both variants (the averages
are finished on their done list).  The variants alternate round by round (interleave what you compare, report the spread):
every round times `steps` steps of each variant in turn; per variant the median over the rounds is reported with min / max and
the coefficient of variation, and NG with the bytes the accumulation pass moves per step: per (env, column) an f32 load, an f64
load and an f64 store — E * NG * (4 + 8 + 8) — plus per env the touched words read, the seen words (read, and written when a
key first exists) and the step count (read and written).  Random actions, device-side auto-reset from a 16-map pool with
max_steps = 128 as in scripts/step_stats_timing.py; all envs restart on the same step, so the timed window (default 256 steps)
is a whole number of episodes and holds two finish passes over all envs.  Prints one JSON line.
Usage (GPU box): python scripts/time_avg_timing.py [envs] [steps] [rounds]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.engine import BatchedMettaGrid  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5

spec = presets.rung3_spec()
spec.max_steps = 128
prog = compile_spec(spec, 32, 32, max_objects=192)
A = prog.num_agents
maps = np.stack([prog.class_map(presets.rung3_map(s)) for s in range(16)])
eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
eng.set_map_pool(maps)
eng.set_auto_reset(True)
eng.set_episode_stats(True)
stream = eng._ext_stream()
gen = torch.Generator(device=eng.actions.device).manual_seed(1)
nact = len(prog.action_names)
acts = [torch.randint(0, nact, (E * A,), generator=gen, device=eng.actions.device, dtype=torch.int32) for _ in range(8)]


def run(n: int) -> None:
    for t in range(n):
        eng.actions.copy_(acts[t % 8])
        eng.vibe_actions.copy_(acts[(t + 3) % 8])
        eng.wait_for_caller()
        eng.step()


run(50)   # warm-up
eng.sync()
VARIANTS = ("off", "on")
ms = {k: [] for k in VARIANTS}
layout = None
for _ in range(rounds):
    for name in VARIANTS:
        eng.set_time_averages(name == "on")
        if name == "on":
            layout = dict(eng._tal)
        run(5)
        eng.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run(steps)
        t1.record(stream)
        t1.synchronize()
        ms[name].append(t0.elapsed_time(t1) / steps)
totals = eng.drain_time_averages()   # (switched on mid-episode every round: the first episode of a window is partial)
eng.set_time_averages(False)
NG, NGW = layout["NG"], layout["SEEN_WORDS"]
out = {"envs": E, "steps": steps, "rounds": rounds, "NG": NG,
       "accum_bytes_per_step": {"values": E * NG * (4 + 8 + 8), "touched_words": E * NGW * 4, "seen_words": E * NGW * 4, "step_counts": E * 8},
       "episodes_last_window": totals["episodes"], "partial_last_window": totals["partial"]}
out["accum_bytes_per_step"]["total"] = sum(out["accum_bytes_per_step"].values())
for name in VARIANTS:
    a = np.asarray(ms[name])
    out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                 "cv_pct": round(float(a.std() / a.mean() * 100), 2), "ms_rounds": [round(float(x), 4) for x in a]}
out["on_minus_off_ms_median"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 4)
print(json.dumps(out), flush=True)
eng.close()
