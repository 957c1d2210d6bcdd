"""BUILD-CONTAINER ONLY — golden replays of the reference's own replay writer.

    python tests/golden/make_replay_fixture.py

Replays the action traces of the committed fixtures ref_chains / ref_spawn_in_event / ref_dynamic_limits
(tests/golden/make_reference_fixtures.py: same configs, seeds, actions and set_inventory calls) on the REFERENCE — its Python
``Simulation`` with an ``InMemoryReplayWriter`` attached (python/src/mettagrid/simulator/replay_log_writer.py) on the reference
C++ engine oracle/_ref — until the episode ends or the trace does, and keeps what ``get_replay_data`` returns without the two
config dumps (``mg_config``, ``policy_env_interface``), plus the resources behind each capacity name.  Output: tests/golden/replay_<scenario>.json (data only).
"""
from __future__ import annotations

import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_fixtures as mrf  # noqa: E402

NAMES = ("chains", "spawn_in_event", "dynamic_limits")
KEEP = ("version", "action_names", "animation_names", "item_names", "type_names", "capacity_names", "tags", "map_size",
        "num_agents", "max_steps", "objects", "infos")


def _stub_policy_env_interface() -> None:
    """The writer dumps a PolicyEnvInterface into the replay; the dump is not kept, and the module's imports may not
    resolve under this Python.  Only that one symbol is replaced, and only when the real import fails."""
    try:
        import mettagrid.policy.policy_env_interface  # noqa: F401
        return
    except Exception:
        pass

    class PolicyEnvInterface:
        @classmethod
        def from_mg_cfg(cls, cfg):
            return cls()

        def model_dump(self, mode="json"):
            return {}

    for k in [k for k in sys.modules if k.startswith("mettagrid.policy")]:
        del sys.modules[k]
    pkg = types.ModuleType("mettagrid.policy")
    pkg.__path__ = []
    mod = types.ModuleType("mettagrid.policy.policy_env_interface")
    mod.PolicyEnvInterface = PolicyEnvInterface
    sys.modules["mettagrid.policy"] = pkg
    sys.modules["mettagrid.policy.policy_env_interface"] = mod


def run(name: str) -> dict:
    import numpy as np
    mrf.import_reference(shim=False)
    _stub_policy_env_interface()
    from mettagrid.simulator import Simulation
    from mettagrid.simulator.replay_log_writer import InMemoryReplayWriter
    from mettagrid.simulator.simulator import Buffers
    cfg, seed, steps, _ = mrf.SCENARIOS[name]()
    z = np.load(os.path.join(HERE, f"ref_{name}.npz"))
    doc = json.load(open(os.path.join(HERE, f"ref_{name}.json")))
    A, T = z["obs"].shape[1], z["obs"].shape[2]
    bufs = Buffers(observations=np.zeros((A, T, 3), np.uint8), terminals=np.zeros(A, bool), truncations=np.zeros(A, bool),
                   rewards=np.zeros(A, np.float32), masks=np.ones(A, bool), actions=np.zeros(A, np.int32),
                   teacher_actions=np.zeros(A, np.int32), vibe_actions=np.zeros(A, np.int32))
    writer = InMemoryReplayWriter()
    sim = Simulation(cfg, seed=seed, event_handlers=[writer], buffers=bufs)
    c = sim._c_sim
    played = 0
    for t in range(min(steps, len(z["actions"]))):
        for when, agent_id, inv in doc.get("set_inventory", []):
            if when == t:
                c.set_inventory(agent_id, {int(k): int(v) for k, v in inv})
        bufs.actions[:] = z["actions"][t]
        bufs.vibe_actions[:] = z["vibe_actions"][t]
        sim.step()
        played = t + 1
        if sim.is_done():
            break
    data = writer._episode_replay.get_replay_data()
    out = {k: data[k] for k in KEEP}
    out["infos"] = {"episode_rewards": [float(x) for x in data["infos"]["episode_rewards"]],
                    "attributes": dict(data["infos"]["attributes"])}
    # which resources each capacity name stands for: the first agent's limit groups (what the writer groups the limits by)
    limits = cfg.game.agents[0].inventory.limits if cfg.game.agents else {}
    out["capacity_resources"] = {cap: [str(r) for r in limits[cap].resources] for cap in sorted(limits)}
    out["scenario"] = name
    out["steps_played"] = played
    return json.loads(json.dumps(out))   # tuples -> lists, numpy scalars refused


def main() -> None:
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        out = run(sys.argv[2])
        json.dump(out, open(os.path.join(HERE, f"replay_{sys.argv[2]}.json"), "w"), separators=(",", ":"), sort_keys=True)
        return
    import subprocess
    for name in NAMES:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "child", name])
        p = os.path.join(HERE, f"replay_{name}.json")
        d = json.load(open(p))
        print(p, os.path.getsize(p), "bytes;", d["steps_played"], "steps;", len(d["objects"]), "objects")


if __name__ == "__main__":
    main()
