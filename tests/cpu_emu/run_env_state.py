"""TEST INFRASTRUCTURE ONLY — save / load / copy of envs' state (mgx_save_envs / mgx_load_envs / mgx_copy_envs) in the
sanitizer build (tests/cpu_emu/libmgx_emu.so, see README.md), world state compared with the oracle after every step.

In this build device memory is host memory, so the record buffer is a numpy array handed to the C entry points directly.
Per scenario: step k, save every env, copy 1 -> 3 and 4 -> 0 (and swap 1 <-> 2), step m against oracles that replay the
sources; then load the saved records into the reversed slots and step m again against oracles of the saved envs.

  python tests/cpu_emu/run_env_state.py [scenario ...]      (default: rung3 dynamic)
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from run_emu import compare, hp, op, use_emu_library, world_state  # noqa: E402
from mettagrid_amd import engine  # noqa: E402


def run(name: str, E: int = 5, k: int = 6, m: int = 6) -> None:
    spec_f, map_f, _, invalid = hp.scenario(name)
    maps = [map_f(s) for s in range(E)]
    prog = hp.compile_scenario(name, spec_f(), *maps[0].shape)
    cms = np.stack([prog.class_map(mp) for mp in maps])
    seeds = np.arange(E, dtype=np.uint32) * 7 + 3
    eng = engine.BatchedMettaGrid(prog, cms, seeds, buffers="host")
    L, A = eng.L, prog.num_agents
    acts = [hp.make_actions(prog, i, k + 2 * m, invalid) for i in range(E)]

    def step(t):
        eng.actions[:] = np.concatenate([a[0][t] for a in acts])
        eng.vibe_actions[:] = np.concatenate([a[1][t] for a in acts])
        eng.step()

    def oracle(src, t0):
        o = op.OracleSim(prog, cms[src], int(seeds[src]))
        o.reinit_buffers()
        for t in range(t0):
            o.step(acts[src][0][t], acts[src][1][t])
        return o

    def check(oracles, t, where):
        succ = eng.action_success()
        for i, o in oracles.items():
            wa = world_state(prog, o.raw_objects(), o.raw_stats(), o.snapshot()["action_success"])
            wb = world_state(prog, eng.raw_objects(i), eng.raw_stats(i), succ[i * A:(i + 1) * A])
            compare(prog, wa, wb, f"{name} {where} env {i} step {t}")

    for t in range(k):
        step(t)
    info = engine.EnvStateInfo()
    assert L.mgx_env_state_info(eng.h, ctypes.byref(info)) == 0
    buf = np.zeros((E, info.record_bytes), np.uint8)
    lst = np.arange(E, dtype=np.int32)
    assert L.mgx_save_envs(eng.h, lst.ctypes.data, E, buf.ctypes.data) == 0, L.mgx_last_error()
    src, dst = np.array([1, 4, 2, 1], np.int32), np.array([3, 0, 1, 2], np.int32)
    assert L.mgx_copy_envs(eng.h, src.ctypes.data, dst.ctypes.data, len(src)) == 0, L.mgx_last_error()
    src_of = {int(d): int(s) for s, d in zip(src, dst)}
    oracles = {i: oracle(src_of.get(i, i), k) for i in range(E)}
    check(oracles, k, "after copy")
    for t in range(k, k + m):
        step(t)
        for i, o in oracles.items():
            o.step(acts[i][0][t], acts[i][1][t])
        check(oracles, t + 1, "copied")
    rev = lst[::-1].copy()   # record j (env j at step k) -> slot E - 1 - j
    assert L.mgx_load_envs(eng.h, rev.ctypes.data, E, buf.ctypes.data, ctypes.byref(info)) == 0, L.mgx_last_error()
    oracles = {int(rev[j]): oracle(j, k) for j in range(E)}
    check(oracles, k, "after load")
    for t in range(k + m, k + 2 * m):
        step(t)
        for i, o in oracles.items():
            o.step(acts[i][0][t], acts[i][1][t])
        check(oracles, t + 1, "loaded")
    bits, first = eng.poll_errors()
    assert bits == 0, f"{name}: env error bits {bits} (first env {first})"
    eng.close()


if __name__ == "__main__":
    use_emu_library()
    for n in sys.argv[1:] or ["rung3", "dynamic"]:
        run(n)
        print("ok", n, flush=True)
