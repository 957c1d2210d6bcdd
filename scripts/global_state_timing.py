"""Cost of the global state rows (mgx_set_global_state): event-timed mean step of the rung-3 (32 x 32, 16 agents) and rung-4
(64 x 64, 64 agents) benchmark shapes with the feature off, on with every class included and on with `wall` excluded, in one
process, one engine per rung.  The variants alternate round by round (interleave what you compare, report the spread): every
round times `steps` steps of each variant in turn; per variant the median over the rounds is reported with min / max and the
coefficient of variation.  For the two "on" variants also the kernel's own time (events around `kernel_reps` back-to-back
passes over all envs, mgx_write_global_state) and the bytes one pass must move — the grid, one object row per object on it
(class, vibe, agent, order word, 32-byte inventory row; extended programs: + 32 bytes of tags and the flag byte) and 4 bytes
per token written — as a fraction of 8 TB/s over the kernel's time.  Random actions, device-side auto-reset from a 16-map pool
with max_steps = 128 as in scripts/step_stats_timing.py.  Prints one JSON line per rung.
Usage (GPU box): python scripts/global_state_timing.py [envs] [steps] [rounds] [rungs, e.g. 34]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.engine import BatchedMettaGrid  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 128
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rungs = sys.argv[4] if len(sys.argv) > 4 else "34"
KERNEL_REPS = 20
VARIANTS = {"off": None, "on_all": (), "on_no_wall": ("wall",)}


def workload(rung: int):
    if rung == 3:
        spec, H, W, S = presets.rung3_spec(), 32, 32, 192
        objs, agents = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}
    else:
        spec, H, W, S = presets.rung4_spec(), 64, 64, presets.RUNG4_MAX_OBJECTS
        objs, agents = dict(presets.RUNG4_OBJECTS), dict(presets.RUNG4_AGENTS)
    spec.max_steps = 128
    prog = compile_spec(spec, H, W, max_objects=S)
    return prog, random_class_maps(prog, H, W, objs, agents, range(16))


def measure(rung: int) -> dict:
    prog, maps = workload(rung)
    A = prog.num_agents
    eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    eng.set_map_pool(maps)
    eng.set_auto_reset(True)
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

    def timed(f) -> float:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        f()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    run(50)   # warm-up
    eng.sync()
    ms = {k: [] for k in VARIANTS}
    kernel_ms = {k: [] for k in VARIANTS if VARIANTS[k] is not None}
    info = {}
    extended = bool(eng.L.mgx_is_extended(eng.h))
    obj_bytes = 2 + 1 + 1 + 8 + 32 + (33 if extended else 0)
    for _ in range(rounds):
        for name, exclude in VARIANTS.items():
            if exclude is None:
                eng.set_global_state(max_tokens=0)
            else:
                tokens, counts, _ = eng.set_global_state(exclude=exclude)
            run(5)
            eng.sync()
            ms[name].append(timed(lambda: run(steps)) / steps)
            if exclude is not None:
                kernel_ms[name].append(timed(lambda: [eng.write_global_state() for _ in range(KERNEL_REPS)]) / KERNEL_REPS)
                eng.sync()
                mean_tokens = float(counts.view(torch.int32).double().mean())
                objects = float((maps != 0).reshape(16, -1).sum(axis=1).mean())   # (every object is read, whatever the filter)
                moved = E * (maps.shape[1] * maps.shape[2] * 2 + objects * obj_bytes + 4 * mean_tokens)
                info[name] = {"row_dwords": int(tokens.shape[1]), "mean_tokens": round(mean_tokens, 1), "max_tokens_seen": int(counts.view(torch.int32).max()),
                              "bytes_per_pass": int(moved)}
    eng.set_global_state(max_tokens=0)
    out = {"rung": rung, "envs": E, "steps": steps, "rounds": rounds}
    for name in VARIANTS:
        a = np.asarray(ms[name])
        out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                     "cv_pct": round(float(a.std() / a.mean() * 100), 2), "ms_rounds": [round(float(x), 4) for x in a]}
        if name in kernel_ms:
            k = np.asarray(kernel_ms[name])
            out[name].update(info[name])
            out[name].update({"kernel_ms_median": round(float(np.median(k)), 4), "kernel_ms_min": round(float(k.min()), 4),
                              "kernel_ms_max": round(float(k.max()), 4),
                              "fraction_of_8TBps": round(info[name]["bytes_per_pass"] / (float(np.median(k)) * 1e-3) / 8e12, 4)})
    eng.close()
    return out


for r in rungs:
    print(json.dumps(measure(int(r))), flush=True)
