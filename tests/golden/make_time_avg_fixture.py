"""BUILD-CONTAINER ONLY — golden `time_averaged_game_stats` of the reference's own TimeAveragedStatsHandler.

    python tests/golden/make_time_avg_fixture.py

Replays the action traces of the committed fixtures ref_navigation / ref_chains (tests/golden/make_reference_fixtures.py:
same configs, seeds, actions and set_inventory calls) on the REFERENCE — its Python ``Simulation`` with its
``TimeAveragedStatsHandler`` attached (python/src/mettagrid/simulator/time_averaged_stats.py:17-41, as runner/rollout.py:107-135
attaches it) and caller buffers bound the way ``MettaGridPufferEnv`` binds them, on the reference C++ engine oracle/_ref —
until the episode ends, and records the handler's ``time_averaged_game_stats`` (floats as ``float.hex()``), the steps played
and the keys the game dict held after step 1.  In neither of the two does a key appear after the first step, so the rung3_s0
golden's scenario is added (``run_golden``: the reference engine through oracle/ref_driver.RefSim, the handler's lines
restated); ``"source"`` says which was done.  That golden's trace is 160 steps and
its episode does not end within them: the fixture is the handler's value after 160 steps (``steps_played``), which pins the
key that first exists mid-episode ("chest.ore") on a run that stops before the episode does; the two reference configs pin the
value at an episode's end.  Output: tests/golden/time_avg_<scenario>.json (data only).
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_fixtures as mrf  # noqa: E402


def _buffers(np, A, T):
    from mettagrid.simulator.simulator import Buffers
    return Buffers(observations=np.zeros((A, T, 3), np.uint8), terminals=np.zeros(A, bool), truncations=np.zeros(A, bool),
                   rewards=np.zeros(A, np.float32), masks=np.ones(A, bool), actions=np.zeros(A, np.int32),
                   teacher_actions=np.zeros(A, np.int32), vibe_actions=np.zeros(A, np.int32))


def run(name: str) -> dict:
    import numpy as np
    mrf.import_reference(shim=False)
    cfg, seed, steps, _ = mrf.SCENARIOS[name]()
    z = np.load(os.path.join(HERE, f"ref_{name}.npz"))
    doc = json.load(open(os.path.join(HERE, f"ref_{name}.json")))
    A, T = z["obs"].shape[1], z["obs"].shape[2]
    first_keys, done_at = None, None
    from mettagrid.simulator import Simulation
    from mettagrid.simulator.time_averaged_stats import TimeAveragedStatsHandler
    handler = TimeAveragedStatsHandler()
    bufs = _buffers(np, A, T)
    sim = Simulation(cfg, seed=seed, event_handlers=[handler], buffers=bufs)
    c = sim._c_sim
    source = "python: Simulation + TimeAveragedStatsHandler"
    for t in range(steps):
        for when, agent_id, inv in doc["set_inventory"]:
            if when == t:
                c.set_inventory(agent_id, {int(k): int(v) for k, v in inv})
        bufs.actions[:] = z["actions"][t]
        bufs.vibe_actions[:] = z["vibe_actions"][t]
        sim.step()
        if t == 0:
            first_keys = sorted(sim.episode_stats.get("game", {}))
        if sim.is_done():
            done_at = t + 1
            break
    ta = dict(handler.time_averaged_game_stats)
    assert done_at is not None, f"{name}: the episode did not end within the fixture's trace"
    out = {"scenario": name, "source": source, "steps_played": done_at, "keys_after_step_1": first_keys,
           "time_averaged_game_stats": {k: float(v).hex() for k, v in ta.items()},
           "late_keys": sorted(set(ta) - set(first_keys))}
    return out


def run_golden(name: str, seed: int) -> dict:
    """A scenario of tests/golden/make_golden.py (<name>_s<seed>.npz), whose config exists only as this project's spec: the
    reference ENGINE is driven through oracle/ref_driver.RefSim over the golden's whole action trace and the handler's lines
    (time_averaged_stats.py:30-41) are applied to ``get_episode_stats()["game"]``."""
    import numpy as np
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import helpers as hp
    import ref_driver as rd
    spec_f, map_f, steps, _ = hp.SCENARIOS[name]
    cells = map_f(seed)
    prog = hp.compile_scenario(name, spec_f(), *cells.shape)
    sim = rd.RefSim(spec_f(), cells, seed, prog)
    z = np.load(os.path.join(HERE, f"{name}_s{seed}.npz"))
    # caller buffers bound the way MettaGridPufferEnv binds them (a second set_buffers: a second initial observation pass)
    A, T = z["obs"].shape[1], z["obs"].shape[2]
    obs, term, trunc, rew = np.zeros((A, T, 3), np.uint8), np.zeros(A, bool), np.zeros(A, bool), np.zeros(A, np.float32)
    act, vact = np.zeros(A, np.int32), np.zeros(A, np.int32)
    sim.c.set_buffers(obs, term, trunc, rew, act, vact)
    count, acc, first_keys = 0, {}, None
    for t in range(steps):
        act[:] = z["actions"][t]
        vact[:] = z["vibe_actions"][t]
        sim.c.step()
        game = sim.c.get_episode_stats().get("game", {})
        count += 1                                   # time_averaged_stats.py:32-35
        for key, value in game.items():
            acc[key] = acc.get(key, 0.0) + float(value)
        if t == 0:
            first_keys = sorted(game)
    ta = {k: v / count for k, v in acc.items()}      # :38-41
    return {"scenario": f"{name}_s{seed}", "steps_played": count, "keys_after_step_1": first_keys,
            "source": "oracle/_ref through ref_driver.RefSim + the handler's lines restated (the scenario has no reference Python config)",
            "time_averaged_game_stats": {k: float(v).hex() for k, v in ta.items()}, "late_keys": sorted(set(ta) - set(first_keys))}


def main() -> None:
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        out = run_golden("rung3", 0) if sys.argv[2] == "rung3_s0" else run(sys.argv[2])
        json.dump(out, open(os.path.join(HERE, f"time_avg_{sys.argv[2]}.json"), "w"), separators=(",", ":"), sort_keys=True)
        return
    import subprocess
    late = 0
    for name in ("navigation", "chains", "rung3_s0"):   # (rung3_s0: chest.* game stats first exist when an agent uses the chest)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "child", name])
        p = os.path.join(HERE, f"time_avg_{name}.json")
        d = json.load(open(p))
        late += len(d["late_keys"])
        print(p, os.path.getsize(p), "bytes;", d["source"], "; ended at step", d["steps_played"], "; keys",
              len(d["time_averaged_game_stats"]), "; absent after step 1:", d["late_keys"])
    # key-existence timing is exercised only if some key appears after the first step
    assert late > 0, "no scenario has a game key that is absent after step 1 and present at the end"


if __name__ == "__main__":
    main()
