"""Time mgx_save_envs / mgx_load_envs / mgx_copy_envs of every env of the rung-3 benchmark shape (32 x 32, 24 agents) and
print one JSON line: record bytes, bytes read + written per call and the rate.  Event timing covers the whole call on the
engine's stream (the env-list upload included); run it under `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python
scripts/env_state_timing.py` for the kernel time alone (mgx_env_state_kernel).
Usage (GPU box): python scripts/env_state_timing.py [envs] [reps]"""
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
maps = np.stack([prog.class_map(presets.rung3_map(s)) for s in range(16)])
eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
for _ in range(3):
    eng.step()
eng.sync()
rec = eng.env_state_info()["record_bytes"]
stream = eng._ext_stream()


def timed(fn) -> float:
    fn()   # warm-up (first call allocates the staging buffers)
    eng.sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


st = eng.save_envs()
half = E // 2
out = {"envs": E, "record_bytes": rec, "reps": reps}
for name, fn, moved in (("save", lambda: eng.save_envs(), 2 * E * rec),
                        ("load", lambda: eng.load_envs(st), 2 * E * rec),
                        ("copy_half", lambda: eng.copy_envs(np.arange(half), np.arange(half, E)), 4 * half * rec)):
    ms = timed(fn)
    out[name] = {"ms": round(ms, 4), "bytes_moved": moved, "GBps": round(moved / ms / 1e6, 1)}
print(json.dumps(out), flush=True)
eng.close()
