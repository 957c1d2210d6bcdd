"""BUILD-CONTAINER ONLY — golden text frames of the reference's own renderer.

    python tests/golden/make_render_fixture.py

What ``MettaGridPufferEnv.render()`` returns (python/src/mettagrid/envs/mettagrid_puffer_env.py:505-524) is
``MapBuffer(DEFAULT_SYMBOL_MAP + game.render.symbols, map_height, map_width).render_full_map(grid_objects())``
(renderer/miniscope/buffer.py, symbol.py).  This script imports the reference from where it lies (the shims and the scenario
table of make_reference_fixtures.py) and records, as data:

  (a) "frames": for the scenarios arena, navigation and spawn_in_event, the recorded action trace of ref_<scenario>.npz (and
      the set_inventory calls of ref_<scenario>.json) replayed on the reference engine; at step 0, one mid step and the last
      step the text frame and the (type_name, r, c, agent_id) list of grid_objects() (agent_id -1: not an agent);
  (b) "synthetic": object lists run through the reference's MapBuffer alone — walls in the interior with an object outside their
      box, no wall, no object, a dotted type name that falls back to its base, an unknown type, overrides of "empty" and of a
      type, agents 9 and 10;
  (c) "default_symbols" and "agent_squares": the reference's tables.

Output: tests/golden/render_frames.json (not ref_*.json: the reference-config tests take every ref_*.json for a scenario).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_fixtures as mrf  # noqa: E402

SCENARIOS = ("arena", "navigation", "spawn_in_event")

SYNTHETIC = [
    # name, H, W, symbol overrides, [(type_name, r, c, agent_id)]
    ("interior_walls", 7, 9, {}, [("wall", 2, 2, -1), ("wall", 2, 5, -1), ("wall", 4, 3, -1), ("crate", 3, 4, -1), ("crate", 0, 0, -1),
                                  ("agent", 3, 3, 0), ("agent", 6, 8, 1)]),
    ("no_wall", 6, 6, {}, [("crate", 1, 2, -1), ("agent", 4, 4, 2), ("crate", 3, 1, -1)]),
    ("no_object", 5, 4, {}, []),
    ("dotted_falls_back", 4, 5, {}, [("wall", 0, 0, -1), ("wall", 3, 4, -1), ("block.heavy", 1, 1, -1), ("block.heavy", 2, 3, -1)]),
    ("unknown_type", 4, 4, {}, [("wall", 0, 0, -1), ("wall", 3, 3, -1), ("mystery", 1, 2, -1), ("crate", 2, 1, -1)]),
    ("overrides", 4, 6, {"empty": "..", "crate": "CC", "wall": "##"},
     [("wall", 0, 0, -1), ("wall", 0, 5, -1), ("wall", 3, 0, -1), ("wall", 3, 5, -1), ("crate", 1, 2, -1), ("mystery", 2, 4, -1),
      ("agent", 2, 2, 3)]),
    ("agents_9_and_10", 3, 6, {}, [("wall", 0, 0, -1), ("wall", 2, 5, -1), ("agent", 1, 1, 9), ("agent", 1, 3, 10), ("agent", 1, 4, 7)]),
]


def object_dicts(rows) -> dict:
    out = {}
    for i, (name, r, c, agent) in enumerate(rows):
        out[i + 1] = {"id": i + 1, "type_name": name, "r": r, "c": c}
        if agent >= 0:
            out[i + 1]["agent_id"] = agent
    return out


def main() -> None:
    mrf.import_reference(shim=False)
    from mettagrid.renderer.miniscope.buffer import MapBuffer
    from mettagrid.renderer.miniscope.symbol import AGENT_SQUARES, DEFAULT_SYMBOL_MAP
    from mettagrid.simulator import Simulation
    doc = {"default_symbols": dict(DEFAULT_SYMBOL_MAP), "agent_squares": list(AGENT_SQUARES), "frames": [], "synthetic": []}
    for name in SCENARIOS:
        cfg, seed, steps, _ = mrf.SCENARIOS[name]()
        z = np.load(os.path.join(HERE, f"ref_{name}.npz"))
        fix = json.load(open(os.path.join(HERE, f"ref_{name}.json")))
        sim = Simulation(cfg, seed=seed)
        c = sim._c_sim
        overrides = dict(cfg.game.render.symbols)
        symbols = dict(DEFAULT_SYMBOL_MAP)
        symbols.update(overrides)
        wanted = sorted({0, steps // 2, steps})

        def record(t):
            objs = c.grid_objects()
            text = MapBuffer(symbol_map=symbols, initial_height=c.map_height, initial_width=c.map_width).render_full_map(objs)
            doc["frames"].append({"scenario": name, "step": t, "height": int(c.map_height), "width": int(c.map_width),
                                  "symbols": overrides, "text": text,
                                  "objects": [[o["type_name"], int(o["r"]), int(o["c"]), int(o.get("agent_id", -1))] for o in objs.values()]})
        if 0 in wanted:
            record(0)
        for t in range(steps):
            for when, agent_id, inv in fix["set_inventory"]:
                if when == t:
                    c.set_inventory(agent_id, dict(map(tuple, inv)))
            c.actions()[:] = z["actions"][t]
            c.vibe_actions()[:] = z["vibe_actions"][t]
            c.step()
            if t + 1 in wanted:
                record(t + 1)
        assert np.array_equal(c.observations(), z["obs"][steps]), f"{name}: the replay left the recorded trace"
    for name, H, W, overrides, rows in SYNTHETIC:
        symbols = dict(DEFAULT_SYMBOL_MAP)
        symbols.update(overrides)
        text = MapBuffer(symbol_map=symbols, initial_height=H, initial_width=W).render_full_map(object_dicts(rows))
        doc["synthetic"].append({"name": name, "height": H, "width": W, "symbols": overrides, "objects": [list(r) for r in rows], "text": text})
    p = os.path.join(HERE, "render_frames.json")
    json.dump(doc, open(p, "w"), ensure_ascii=False, indent=0, separators=(",", ":"))
    print(p, os.path.getsize(p), "bytes;", len(doc["frames"]), "scenario frames,", len(doc["synthetic"]), "synthetic cases")


if __name__ == "__main__":
    main()
