"""Cost of the replay recorder: event-timed mean step of the rung-3 benchmark shape (32 x 32, 16 agents) with 0, 64 and
1 024 watched envs, in one process on one engine, and the bytes logged per watched env-step.  The variants alternate round
by round (interleave what you compare, report the spread): every round times `steps` steps of each
variant in turn; per variant the median over the rounds is reported with min / max and the coefficient of variation.
Random actions, device-side auto-reset from a 16-map pool with max_steps = 128, so episodes end and keyframes are part of the
cost; all envs restart on the same step, so the timed window is a whole number of episodes (default 256 steps: two mass
restarts in every window, whatever its phase).  Prints one JSON line.  Usage (GPU box): python scripts/replay_timing.py [envs] [steps] [rounds]"""
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
WATCH = (0, 64, 1024)

spec = presets.rung3_spec()
spec.max_steps = 128
prog = compile_spec(spec, 32, 32, max_objects=192)
maps = np.stack([prog.class_map(presets.rung3_map(s)) for s in range(16)])
eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
eng.set_map_pool(maps)
eng.set_auto_reset(True)
stream = eng._ext_stream()
gen = torch.Generator(device=eng.actions.device).manual_seed(1)
nact = len(prog.action_names)
acts = [torch.randint(0, nact, (E * prog.num_agents,), generator=gen, device=eng.actions.device, dtype=torch.int32) for _ in range(8)]


def run(n: int) -> None:
    for t in range(n):
        eng.actions.copy_(acts[t % 8])
        eng.vibe_actions.copy_(acts[(t + 3) % 8])
        eng.wait_for_caller()
        eng.step()


def watch(n: int) -> None:
    eng.set_replay(np.linspace(0, E - 1, n).astype(np.int64) if n else [], words_per_env=1 << 16)


run(50)   # warm-up
eng.sync()
ms = {n: [] for n in WATCH}
logged = {n: 0 for n in WATCH}
overflow = {n: 0 for n in WATCH}
for _ in range(rounds):
    for n in WATCH:
        watch(n)
        run(5)
        eng.sync()
        if n:
            eng.drain_replay()   # the keyframe every freshly watched env starts with is not part of the steady state
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run(steps)
        t1.record(stream)
        t1.synchronize()
        ms[n].append(t0.elapsed_time(t1) / steps)
        if n:
            words, flags = eng.drain_replay()
            logged[n] += sum(len(w) for w in words) * 4
            overflow[n] += sum(1 for f in flags if f & 1)
watch(0)
out = {"envs": E, "steps": steps, "rounds": rounds}
for n in WATCH:
    a = np.asarray(ms[n])
    out[f"watched_{n}"] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                           "cv_pct": round(float(a.std() / a.mean() * 100), 2), "ms_rounds": [round(float(x), 4) for x in a]}
    if n:
        out[f"watched_{n}"]["bytes_per_env_step"] = round(logged[n] / (n * steps * rounds), 1)
        out[f"watched_{n}"]["overflowed_envs"] = overflow[n]
print(json.dumps(out), flush=True)
eng.close()
