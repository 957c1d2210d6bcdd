"""Cost of the per-step stat readout (mgx_set_step_stats): event-timed mean step of the rung-3 benchmark shape (32 x 32, 16
agents) with no keys, 2 game + 4 agent keys and 8 game + 16 agent keys, in one process on one engine.  The variants alternate
round by round (interleave what you compare, report the spread): every round times `steps` steps of each variant in turn; per
variant the median over the rounds is reported with min / max and the coefficient of variation, and for the keyed variants the
bytes the readout moves per step: the output tensors, plus the 128-byte lines its columns read (per agent one line of the stat
row for every distinct line its stat columns fall into, the touched word's line, the 32-byte counter record's line, one line of
16 agents' words per coverage / reward array; per env the game row's and the touched word's lines).  Random actions, device-side
auto-reset from a 16-map pool with max_steps = 128 as in scripts/replay_timing.py; all envs restart on the same step, so the
timed window (default 256 steps) is a whole number of episodes.  Prints one JSON line.
Usage (GPU box): python scripts/step_stats_timing.py [envs] [steps] [rounds]"""
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

GAME_8 = ["objects.wall", "tokens_written", "attributes/steps", "objects.extractor", "chest.ore", "objects.chest", "tokens_dropped",
          "tokens_free_space"]
AGENT_16 = ["action.move.success", "reward_step", "cell.unique_visited", "ore.gained", "action.failed", "status.max_steps_without_motion",
            "cell.max_distance_from_spawn", "reward_episode", "action.noop.success", "action.change_vibe.success", "ore.amount",
            "energy.amount", "hp.amount", "ore.lost", "ore.deposited", "cell.visited"]
VARIANTS = {"no_keys": ([], []), "g2_a4": (GAME_8[:2], AGENT_16[:4]), "g8_a16": (GAME_8, AGENT_16)}

spec = presets.rung3_spec()
spec.max_steps = 128
prog = compile_spec(spec, 32, 32, max_objects=192)
A = prog.num_agents
maps = np.stack([prog.class_map(presets.rung3_map(s)) for s in range(16)])
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


def bytes_moved(game_keys, agent_keys) -> dict:
    """Output bytes and 128-byte lines read per step, from the resolved columns."""
    gk, ak = eng.step_stats_columns()
    aid = {n: i for i, n in enumerate(prog.agent_stat_names)}
    gid = {n: i for i, n in enumerate(prog.game_stat_names)}
    out = E * len(gk) * 5 + E * A * len(ak) * 5
    stat_lines = {aid[k] // 32 for k, kind in zip(agent_keys, ak) if kind == "stat"}
    touched = any(kind in ("stat", "counter", "cov_unique", "cov_maxdist") for kind in ak)
    per_agent = 128 * (len(stat_lines) + (1 if touched else 0) + (1 if "counter" in ak else 0))
    shared = sum(1 for kind in ("cov_unique", "cov_maxdist", "reward_step", "reward_episode") if kind in ak)   # 4-byte words: 32 agents a line
    game_lines = {gid[k] // 32 for k, kind in zip(game_keys, gk) if kind == "stat"}
    per_env = 128 * (len(game_lines) + (1 if game_lines else 0)) + (4 if "steps" in gk else 0)
    read = E * A * per_agent + E * A * 4 * shared + E * per_env
    return {"output_bytes": out, "read_line_bytes": read, "agent_kinds": ak, "game_kinds": gk}


run(50)   # warm-up
eng.sync()
ms = {k: [] for k in VARIANTS}
moved = {}
for _ in range(rounds):
    for name, (gkeys, akeys) in VARIANTS.items():
        eng.set_step_stats(gkeys, akeys)
        if gkeys or akeys:
            moved[name] = bytes_moved(gkeys, akeys)
        run(5)
        eng.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run(steps)
        t1.record(stream)
        t1.synchronize()
        ms[name].append(t0.elapsed_time(t1) / steps)
eng.set_step_stats([], [])
out = {"envs": E, "steps": steps, "rounds": rounds, "integer_bookkeeping": eng.integer_bookkeeping}
for name in VARIANTS:
    a = np.asarray(ms[name])
    out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                 "cv_pct": round(float(a.std() / a.mean() * 100), 2), "ms_rounds": [round(float(x), 4) for x in a]}
    out[name].update(moved.get(name, {}))
print(json.dumps(out), flush=True)
eng.close()
