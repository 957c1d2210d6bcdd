"""CPU: the host side of the replay recorder (mettagrid_amd/replay.py).

(a) ``encode_step`` -> ``ReplayAssembler`` round trips on synthetic snapshot sequences, one case per series rule of the
    reference's writer (python/src/mettagrid/simulator/replay_log_writer.py).
(b) The CPU oracle stepped through three reference fixtures; its per-step raw objects, rewards and action_success go through
    ``encode_step`` -> ``ReplayAssembler`` and the ``objects`` must equal what the reference's own writer recorded
    (tests/golden/replay_*.json, made by tests/golden/make_replay_fixture.py).  The oracle exposes neither the executed action
    nor effective limits... the latter are restated from the program, so only the keys below are left out."""
import json
import os

import numpy as np
import pytest

import oracle_py as op
import ref_tree
from mettagrid_amd import from_reference as fr
from mettagrid_amd import replay as rp
from mettagrid_amd import spec as S
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.fmt import K

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("chains", "spawn_in_event", "dynamic_limits")
ORACLE_EXCLUDED = {"animation_id", "action_id", "inventory_capacities"}


def drop(objects, keys):
    return [{k: v for k, v in o.items() if k not in keys} for o in objects]


# ---- (a) synthetic sequences ---------------------------------------------------------------------------------------------
def tiny_prog():
    agent = S.AgentSpec(team_id=0, inventory=S.Inventory(initial={}, default_limit=50,
                                                          limits=[S.Limit(["ore"], base=5, max=40, modifiers={"gear": 10})]))
    spec = S.GameSpec(resource_names=["ore", "gear"], agents=[agent],
                      objects={"wall": S.ObjectSpec(name="wall"), "box": S.ObjectSpec(name="box", inventory=S.Inventory(initial={}, default_limit=9))})
    return compile_spec(spec, 4, 5, max_objects=6)


def record(prog, slot, cell, r, c, alive=1, agent=-1, vibe=0, inv=(), tags=None):
    """A raw object record (include/mgx.h mgx_get_objects) of class ``cell``; ``inv``: (item, amount) in iteration order."""
    rec = np.zeros(42, np.int32)
    cls = prog.class_cells.index(cell)
    rec[:8] = [slot + 1, cls, r, c, vibe, alive, agent, len(inv)]
    rec[8:21] = -1
    for k, (item, amount) in enumerate(inv):
        rec[8 + k] = item
        rec[21 + item] = amount
    coff = int(prog.words[K.H_SECTION_BASE + 2 * K.SEC_CLASSES])
    rec[34:42] = prog.words[coff + cls * K.C_WORDS + K.C_TAGS: coff + cls * K.C_WORDS + K.C_TAGS + 8] if tags is None else tags
    return rec


def snap(objs, step, reward=0.0, executed=0, success=False, done=False):
    return {"objects": objs, "rewards": np.array([reward], np.float32), "executed": np.array([executed], np.int32),
            "success": np.array([success]), "step": step, "terminals": np.array([False]), "truncations": np.array([done])}


def agent_cell(prog):
    return next(c for c in prog.class_cells if c.startswith("agent"))


def assemble(prog, snaps, cut=None):
    sh = rp.Shadow(prog)
    words = [rp.encode_step(sh, s) for s in snaps]
    asm = rp.ReplayAssembler(prog)
    if cut is None:
        return asm.feed(np.concatenate(words)), words
    out = asm.feed(np.concatenate(words[:cut]))
    return out + asm.feed(np.concatenate(words[cut:])), words


def test_keyframe_then_only_changes_and_single_entry_series_collapse():
    prog = tiny_prog()
    ag = agent_cell(prog)
    s0 = [record(prog, 0, "wall", 0, 0), record(prog, 1, ag, 1, 1, agent=0)]
    s1 = [record(prog, 0, "wall", 0, 0), record(prog, 1, ag, 1, 2, agent=0)]
    eps, words = assemble(prog, [snap(s0, 1), snap(s1, 2, executed=4, success=True), snap(s1, 3, executed=4, success=True, done=True)])
    assert int(words[0][0]) == (K.RPL_STEP | K.RPL_F_KEYFRAME) and int(words[1][0]) == K.RPL_STEP
    assert int(words[2][2]) == 0 and int(words[2][3]) & 0xFFFF0000 == K.RPL_END      # nothing changed in step 3: no event, END follows
    (ep,) = eps
    wall, agent = ep["objects"]
    assert wall == {"id": 1, "alive": True, "type_name": "wall", "location": [0, 0], "orientation": 0, "inventory": [], "inventory_max": 0,
                    "inventory_capacities": [], "color": 0, "tag_ids": wall["tag_ids"]}   # every series has one entry: bare values
    assert agent["location"] == [[0, [1, 1]], [1, [2, 1]]] and agent["action_id"] == [[0, 0], [1, 4]]
    assert agent["action_success"] == [[0, False], [1, True]] and agent["alive"] is True and agent["agent_id"] == 0
    assert ep["max_steps"] == 3 and ep["infos"]["attributes"]["steps"] == 3 and ep["version"] == 4


def test_key_first_seen_after_step_0_gets_a_default_entry_at_0():
    prog = tiny_prog()
    ag = agent_cell(prog)
    eps, _ = assemble(prog, [snap([record(prog, 0, "box", 2, 2)], 1),
                             snap([record(prog, 0, "box", 2, 2), record(prog, 1, ag, 1, 1, agent=0, vibe=0)], 2, reward=0.5, done=True)])
    late = eps[0]["objects"][1]
    assert late["alive"] == [[0, False], [1, True]]                 # an object first seen after step 0 starts not alive
    assert late["location"] == [[0, []], [1, [1, 1]]] and late["type_name"] == [[0, ""], [1, "agent"]]
    assert late["current_reward"] == [[0, 0.0], [1, 0.5]] and late["id"] == [[0, 0], [1, 2]]


def test_vanished_object_and_unseen_non_static_objects_turn_not_alive_but_walls_stay():
    prog = tiny_prog()
    s0 = [record(prog, 0, "wall", 0, 0), record(prog, 1, "box", 2, 2, inv=[(0, 3)])]
    s1 = [record(prog, 0, "wall", 0, 0), record(prog, 1, "box", 2, 2, alive=0, inv=[(0, 3)])]
    eps, words = assemble(prog, [snap(s0, 1), snap(s1, 2), snap(s1, 3, done=True)])
    wall, box = eps[0]["objects"]
    assert wall["alive"] is True                                    # static: absent after step 0, never marked dead
    assert box["alive"] == [[0, True], [1, False]] and box["inventory"] == [[0, 3]]
    assert int(words[1][2]) == 1 + 2                                # one event: header + the CORE group


def test_a_slot_dead_at_the_keyframe_is_logged_in_full_when_it_turns_alive():
    prog = tiny_prog()
    dead = [record(prog, 0, "box", 0, 0), record(prog, 1, "box", 2, 2, alive=0, inv=[(0, 3)])]
    live = [record(prog, 0, "box", 0, 0), record(prog, 1, "box", 2, 2, alive=1, inv=[(0, 3)])]
    eps, words = assemble(prog, [snap(dead, 1), snap(live, 2), snap(live, 3, done=True)])
    (slot, mask, _), = rp.parse_words(words[1])[0][3]
    assert slot == 1 and mask == rp.ALL_OBJECT_GROUPS           # not CORE alone: the reader knows nothing of the slot yet
    box = eps[0]["objects"][1]
    assert box["alive"] == [[0, False], [1, True]] and box["inventory"] == [[0, []], [1, [[0, 3]]]]
    assert box["tag_ids"][-1][1] == eps[0]["objects"][0]["tag_ids"] and box["location"] == [[0, []], [1, [2, 2]]]


def test_vanished_key_falls_back_to_its_default():
    prog = tiny_prog()
    ag = agent_cell(prog)
    # slot 1 is an agent, then (another state loaded over it) a plain box: the agent-only keys vanish
    eps, _ = assemble(prog, [snap([record(prog, 0, "box", 0, 0), record(prog, 1, ag, 1, 1, agent=0, vibe=3)], 1, reward=1.5),
                             snap([record(prog, 0, "box", 0, 0), record(prog, 1, "box", 1, 1)], 2, done=True)])
    obj = eps[0]["objects"][1]
    assert obj["vibe"] == [[0, 3], [1, 0]] and obj["current_reward"] == [[0, 1.5], [1, 0.0]] and obj["is_agent"] == [[0, True], [1, 0]]
    assert obj["vision_size"] == [[0, 13], [1, 0]] and obj["type_name"] == [[0, "agent"], [1, "box"]]


def test_inventory_keys_are_the_order_list_and_limits_follow_modifiers():
    prog = tiny_prog()
    ag = agent_cell(prog)
    eps, _ = assemble(prog, [snap([record(prog, 0, ag, 1, 1, agent=0, inv=[(1, 0), (0, 4)])], 1),      # gear present with amount 0
                             snap([record(prog, 0, ag, 1, 1, agent=0, inv=[(1, 2), (0, 4)])], 2, done=True)])
    a = eps[0]["objects"][0]
    assert a["inventory"] == [[0, [[0, 4], [1, 0]]], [1, [[0, 4], [1, 2]]]]
    assert eps[0]["capacity_names"] == ["ore"]
    assert a["inventory_capacities"] == [[0, [[0, 5]]], [1, [[0, 20]]]]     # min 5, 10 per gear held, max 40


def test_total_reward_is_a_float64_sum_of_the_float32_step_rewards():
    prog = tiny_prog()
    ag = agent_cell(prog)
    rewards = [0.1, 0.7, 1e-8, 0.3]
    snaps = [snap([record(prog, 0, ag, 1, 1, agent=0)], t + 1, reward=r, done=t == 3) for t, r in enumerate(rewards)]
    eps, _ = assemble(prog, snaps)
    want = np.cumsum(np.asarray(rewards, np.float32).astype(np.float64))
    assert eps[0]["objects"][0]["total_reward"] == [[t, float(v)] for t, v in enumerate(want)]
    assert eps[0]["infos"]["episode_rewards"] == [float(want[-1])]


def test_two_episodes_across_drains_and_a_partial_third():
    prog = tiny_prog()
    ag = agent_cell(prog)
    snaps = [snap([record(prog, 0, ag, 1, 1 + (t % 2), agent=0)], t % 3 + 1, done=t % 3 == 2) for t in range(8)]
    whole, words = assemble(prog, snaps)
    assert len(whole) == 2 and [int(w[0]) & 1 for w in words] == [1, 0, 0, 1, 0, 0, 1, 0]
    for cut in (1, 3, 4, 7):
        assert assemble(prog, snaps, cut=cut)[0] == whole


def test_a_step_that_does_not_fit_is_dropped_and_the_env_waits_for_its_next_episode():
    prog = tiny_prog()
    ag = agent_cell(prog)
    sh = rp.Shadow(prog)
    s = [record(prog, 0, ag, 1, 1, agent=0)]
    assert len(rp.encode_step(sh, snap(s, 1), room=10)) == 0 and sh.muted and sh.overflow
    assert len(rp.encode_step(sh, snap(s, 2, done=True), room=100)) == 0 and not sh.muted and sh.keyframe_next
    w = rp.encode_step(sh, snap(s, 1), room=100)
    assert int(w[0]) == (K.RPL_STEP | K.RPL_F_KEYFRAME)


def test_write_replay_round_trips(tmp_path):
    doc = {"version": 4, "objects": [{"id": 1}]}
    for ext in (".json.z", ".json.gz", ".json"):
        p = str(tmp_path / ("r" + ext))
        rp.write_replay(doc, p)
        assert rp.read_replay(p) == doc
    import zlib
    assert json.loads(zlib.decompress(open(str(tmp_path / "r.json.z"), "rb").read())) == doc


# ---- (b) the oracle through the reference fixtures -----------------------------------------------------------------------
def load(name):
    doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
    z = np.load(os.path.join(HERE, "golden", f"ref_{name}.npz"))
    gold = json.load(open(os.path.join(HERE, "golden", f"replay_{name}.json")))
    cells = np.asarray(doc["map"], dtype=object)
    prog = fr.compile_reference_config(ref_tree.load(doc["config"]), *cells.shape)
    return doc, z, gold, cells, prog


@pytest.mark.parametrize("name", NAMES)
def test_oracle_replay_equals_the_reference_writers(name):
    doc, z, gold, cells, prog = load(name)
    o = op.OracleSim(prog, prog.class_map(cells), doc["seed"])
    sh = rp.Shadow(prog)
    asm = rp.ReplayAssembler(prog, capacity_groups=gold["capacity_resources"], seed=doc["seed"])
    eps = []
    for t in range(gold["steps_played"]):
        for when, agent_id, inv in doc["set_inventory"]:
            if when == t:
                o.set_inventory(agent_id, dict(map(tuple, inv)))
        o.step(z["actions"][t], z["vibe_actions"][t])
        s = o.snapshot()
        eps += asm.feed(rp.encode_step(sh, {"objects": o.raw_objects(), "rewards": s["rewards"], "executed": np.zeros(prog.num_agents, np.int32),
                                            "success": s["action_success"], "step": o.current_step, "terminals": s["terminals"],
                                            "truncations": s["truncations"]}))
    ep = eps[0] if eps else asm.partial()
    assert drop(ep["objects"], ORACLE_EXCLUDED) == drop(gold["objects"], ORACLE_EXCLUDED)
    assert ep["infos"]["episode_rewards"] == gold["infos"]["episode_rewards"]
    assert ep["max_steps"] == gold["max_steps"] and ep["map_size"] == gold["map_size"] and ep["num_agents"] == gold["num_agents"]
    assert ep["capacity_names"] == gold["capacity_names"] and ep["item_names"] == gold["item_names"]
    assert ep["action_names"] == gold["action_names"] and ep["type_names"] == [n for n in gold["type_names"] if n]
