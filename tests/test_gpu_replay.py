"""GPU: the on-device replay recorder (include/mgx.h mgx_set_replay / mgx_drain_replay; csrc/mgx_replay.h).

Golden replays of the reference's writer, the kernel's words against their numpy restatement bit for bit, episode
boundaries, overflow, isolation from the rest of the step and save / load / copy onto a watched env."""
import json
import os

import numpy as np
import pytest

import ref_tree
from mettagrid_amd import from_reference as fr
from mettagrid_amd import presets
from mettagrid_amd import replay as rp
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.fmt import K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("chains", "spawn_in_event", "dynamic_limits")
EXCLUDED = {"animation_id"}


def drop(objects, keys):
    return [{k: v for k, v in o.items() if k not in keys} for o in objects]


# ---- (c) golden ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_assembled_replay_equals_the_reference_writers(name):
    doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
    z = np.load(os.path.join(HERE, "golden", f"ref_{name}.npz"))
    gold = json.load(open(os.path.join(HERE, "golden", f"replay_{name}.json")))
    cells = np.asarray(doc["map"], dtype=object)
    prog = fr.compile_reference_config(ref_tree.load(doc["config"]), *cells.shape)
    eng = BatchedMettaGrid(prog, prog.class_map(cells)[None], [doc["seed"]], buffers="device", specialize=False)
    eng.set_replay([0])
    for t in range(gold["steps_played"]):
        for when, agent_id, inv in doc["set_inventory"]:
            if when == t:
                eng.set_inventory(0, agent_id, dict(map(tuple, inv)))
        eng.actions.copy_(_dev(eng, z["actions"][t]))
        eng.vibe_actions.copy_(_dev(eng, z["vibe_actions"][t]))
        eng.step(check_errors=True)
    (words,), (flags,) = eng.drain_replay()
    assert not flags & K.RPL_ENV_OVERFLOW
    asm = rp.ReplayAssembler(prog, capacity_groups=gold["capacity_resources"], seed=doc["seed"])
    eps = asm.feed(words)
    ep = eps[0] if eps else asm.partial()
    assert drop(ep["objects"], EXCLUDED) == drop(gold["objects"], EXCLUDED)
    assert ep["infos"]["episode_rewards"] == gold["infos"]["episode_rewards"]
    assert ep["max_steps"] == gold["max_steps"] and ep["capacity_names"] == gold["capacity_names"]


def _dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(eng.actions.device)


# ---- shared: two identical engines in lockstep, one watched, the other restated -------------------------------------------
def small_lean(max_steps=0):
    spec = presets.rung3_spec()
    red = [a for a in spec.agents if a.team_id == 0][:2]
    blue = [a for a in spec.agents if a.team_id != 0][:2]
    spec.agents = red + blue
    spec.max_steps = max_steps
    return spec, ["agent.red", "agent.red", "agent.blue", "agent.blue"]


def edge_cells(agent_names, ranks, extras, H=20, W=20):
    """A HxW map of walls in which the objects of scan-order rank ``ranks`` are agents (object slot = rank); the two cells
    south of each are empty, the third is one of ``extras``; agents beyond ``ranks`` go behind the last one."""
    cells = np.full((H, W), "wall", dtype=object)
    flat = cells.reshape(-1)
    for k, name in enumerate(agent_names):
        occupied = [i for i in range(H * W) if flat[i] != "empty"]
        i = occupied[ranks[k]] if k < len(ranks) else occupied[ranks[-1] + 2 * (k - len(ranks) + 1)]
        flat[i] = name
        r, c = divmod(i, W)
        for dr in (1, 2):
            if r + dr < H:
                cells[r + dr, c] = "empty"
        if r + 3 < H and extras:
            cells[r + 3, c] = extras[k % len(extras)]
    return cells


class Lockstep:
    """Engine ``a`` records ``watched``; engine ``b`` (same program, maps, seeds, actions) supplies the snapshots that
    ``encode_step`` restates."""

    def __init__(self, prog, cms, seeds, watched, words_per_env=None, setup=None):
        self.prog, self.watched = prog, list(watched)
        self.a = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
        self.b = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
        for e in (self.a, self.b):
            if setup:
                setup(e)
        self.a.set_replay(self.watched, words_per_env=words_per_env)
        self.cap = self.a.replay_layout()["WORDS_PER_ENV"]
        self.shadows = [rp.Shadow(prog) for _ in self.watched]
        self.want = [[] for _ in self.watched]
        self.used = [0] * len(self.watched)
        self.rng = np.random.RandomState(7)

    def step(self, n=1):
        import torch
        A, E = self.prog.num_agents, self.a.E
        nact = len(self.prog.action_names)
        for _ in range(n):
            act = torch.as_tensor(self.rng.randint(0, nact, E * A).astype(np.int32)).to(self.a.actions.device)
            vib = torch.as_tensor(self.rng.randint(0, nact, E * A).astype(np.int32)).to(self.a.actions.device)
            for e in (self.a, self.b):
                e.actions.copy_(act)
                e.vibe_actions.copy_(vib)
                e.step(check_errors=True)
            self.restate()

    def restate(self):
        b, A = self.b, self.prog.num_agents
        snap, ex, steps = b.snapshot(), b.executed_actions(), b.current_steps()
        for k, (env, raw) in enumerate(zip(self.watched, b.raw_objects_batch(self.watched))):
            sl = slice(env * A, (env + 1) * A)
            w = rp.encode_step(self.shadows[k], {"objects": raw, "rewards": snap["rewards"][sl], "executed": ex[sl],
                                                 "success": snap["action_success"][sl], "step": int(steps[env]),
                                                 "terminals": snap["terminals"][sl], "truncations": snap["truncations"][sl]},
                               room=self.cap - self.used[k])
            self.used[k] += len(w)
            self.want[k].append(w)

    def drain(self):
        """(drained words, restated words, flags) per watched env since the last drain."""
        words, flags = self.a.drain_replay()
        want = [np.concatenate(w) if w else np.zeros(0, np.uint32) for w in self.want]
        self.want = [[] for _ in self.watched]
        self.used = [0] * len(self.watched)
        for s in self.shadows:
            s.overflow = False
        return words, want, flags


def build(spec_names, H=20, W=20, ranks=(63, 64, 255, 256)):
    spec, names = spec_names
    prog = compile_spec(spec, H, W)
    extras = [n for n in ("extractor", "chest") if n in prog.cell_to_class]
    return prog, prog.class_map(edge_cells(names, ranks, extras, H, W))


# ---- (d) kernel vs restatement ---------------------------------------------------------------------------------------------
def check_against_restatement(ls, watched, steps=32):
    ls.step(steps)
    words, want, flags = ls.drain()
    for k, env in enumerate(watched):
        assert flags[k] == 0 and len(words[k]) > 0
        assert np.array_equal(words[k], want[k]), f"env {env}: the kernel's words differ from encode_step"
    parsed = rp.parse_words(words[0])
    assert [p[0] for p in parsed] == ["step"] * steps and parsed[0][1] == K.RPL_F_KEYFRAME and all(p[1] == 0 for p in parsed[1:])
    assert sum(len(p[3]) for p in parsed[1:]) > 0      # something changed behind the keyframe


def test_drained_words_equal_the_restatement_bit_for_bit_lean():
    """E = 70, watched envs both sides of the world kernel's 64-env workgroup; a 20x20 map with the default 400 object slots
    (the chunk loop runs twice) and agents on slots 63, 64, 255, 256: the wavefront and chunk edges of the scan."""
    prog, cm = build(small_lean())
    E, watched = 70, [0, 63, 64, 69]
    ls = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32) + 11, watched)
    assert not ls.a.L.mgx_is_extended(ls.a.h)
    raw = ls.b.raw_objects(0)
    assert prog.max_objects == 400 and all(raw[s][6] >= 0 for s in (63, 64, 255, 256))
    check_against_restatement(ls, watched)


def small_extended():
    """An 8-agent cut-down of the rung-4 preset: dynamic tags, static and mobile AoE, territory, events, queries."""
    spec = presets.rung4_spec()
    by_team = {}
    for a in spec.agents:
        by_team.setdefault(a.team_id, []).append(a)
    spec.agents = [a for t in sorted(by_team) for a in by_team[t][:2]]
    return spec, ["agent." + presets.RUNG4_TEAMS[t] for t in sorted(by_team) for _ in range(2)]


@pytest.mark.parametrize("sources", [True, False])
def test_drained_words_equal_the_restatement_bit_for_bit_extended(sources):
    """The extended program on the same kind of map: 400 slots, agents on slots 63, 64, 255, 256, so obj_tags, obj_flags
    and limits that move are read at the wavefront and chunk edges of the scan.  ``sources``: healers (static AoE) and flags
    (territory sources) stand below the agents; without them the program's territory type has no source on any create map
    (the engine then keeps room for one: mgx_plan.h)."""
    spec_names = small_extended()
    prog = compile_spec(spec_names[0], 20, 20)
    extras = [n for n in ("healer_red", "flag_red", "healer_blue", "flag_blue", "extractor", "chest") if n in prog.cell_to_class]
    assert len(extras) >= 4
    cm = prog.class_map(edge_cells(spec_names[1], (63, 64, 255, 256), extras if sources else extras[-2:]))
    E, watched = 70, [0, 63, 64, 69]
    ls = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32) + 11, watched)
    assert ls.a.L.mgx_is_extended(ls.a.h)
    raw = ls.b.raw_objects(0)
    assert prog.max_objects == 400 and all(raw[s][6] >= 0 for s in (63, 64, 255, 256))
    check_against_restatement(ls, watched)


# ---- (e) episode boundaries --------------------------------------------------------------------------------------------------
def auto_reset_setup(pool):
    def setup(e):
        e.set_map_pool(pool)
        e.set_auto_reset(True)
    return setup


def test_episode_boundaries_keyframes_and_split_drains():
    prog, cm = build(small_lean(max_steps=8), ranks=(10, 11, 40, 41))
    _, cm2 = build(small_lean(max_steps=8), ranks=(20, 21, 50, 51))
    E, watched = 4, [0, 3]
    pool = np.stack([cm, cm2])
    one = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32), watched, setup=auto_reset_setup(pool))
    two = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32), watched, setup=auto_reset_setup(pool))
    one.step(20)
    w1, want1, f1 = one.drain()
    two.step(5)
    wa, _, _ = two.drain()
    two.step(15)
    wb, _, _ = two.drain()
    for k in range(len(watched)):
        assert np.array_equal(w1[k], want1[k])
        assert np.array_equal(np.concatenate([wa[k], wb[k]]), w1[k])
        parsed = rp.parse_words(w1[k])
        kinds = [(p[0], p[1]) for p in parsed]
        ends = [i for i, p in enumerate(parsed) if p[0] == "end"]
        assert len(ends) == 2 and all(parsed[i][1] in (K.RPL_E_TERMINAL, K.RPL_E_TRUNCATED) and parsed[i][2] == 8 for i in ends)
        assert kinds[0] == ("step", K.RPL_F_KEYFRAME) and all(kinds[i + 1] == ("step", K.RPL_F_KEYFRAME) for i in ends)
        assert sum(1 for p in parsed if p[0] == "step") == 20 and f1[k] == 0
        whole = rp.ReplayAssembler(prog)
        eps = whole.feed(w1[k])
        split = rp.ReplayAssembler(prog)
        eps2 = split.feed(wa[k]) + split.feed(wb[k])
        assert len(eps) == 2 and eps == eps2 and all(e["max_steps"] == 8 for e in eps)
        assert whole.partial()["max_steps"] == 4 and whole.partial() == split.partial()


# ---- (f) overflow --------------------------------------------------------------------------------------------------------------
def test_overflow_drops_whole_steps_and_stays_inside_the_env_region():
    spec_names = small_lean(max_steps=8)
    prog = compile_spec(spec_names[0], 20, 20)
    names = spec_names[1]
    big = edge_cells(names, (10, 11, 40, 41), ["extractor", "chest"])     # ~390 objects: a keyframe logs the walls too
    small = np.full((20, 20), "empty", dtype=object)
    small[1, 1:5] = names
    small[3, 1] = "extractor"
    cm_big, cm_small = prog.class_map(big), prog.class_map(small)
    full = 1 + K.RPL_SLOT_WORDS                            # the largest event
    # B: a keyframe of 5 objects, then 8 steps in which all 5 objects may change in full, and the END marker
    cap = K.RPL_STEP_WORDS + 5 * full + 8 * (K.RPL_STEP_WORDS + 5 * full) + K.RPL_END_WORDS
    assert cap < (full - 2) * int((cm_big > 0).sum())      # (a live non-agent slot's keyframe event has no AGENT group)
    pool = np.stack([cm_small, cm_small])
    ls = Lockstep(prog, np.stack([cm_big, cm_small]), np.array([3, 4], np.uint32), [0, 1], words_per_env=cap,
                  setup=auto_reset_setup(pool))
    ls.step(8)                                             # episode 1 ends in both
    words, want, flags = ls.drain()
    assert flags[0] & K.RPL_ENV_OVERFLOW and len(words[0]) == 0
    assert not flags[1] & K.RPL_ENV_OVERFLOW and len(words[1]) > 0 and np.array_equal(words[1], want[1])
    ls.step(3)                                             # episode 2 from the small pool map: A logs again, keyframe first
    words, want, flags = ls.drain()
    for k in (0, 1):
        assert not flags[k] & K.RPL_ENV_OVERFLOW and np.array_equal(words[k], want[k])
        assert int(words[k][0]) == (K.RPL_STEP | K.RPL_F_KEYFRAME)


# ---- (g) isolation -----------------------------------------------------------------------------------------------------------
def test_a_watch_list_changes_nothing_else():
    prog, cm = build(small_lean())
    E = 70
    ls = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32), [0, 63, 64, 69])
    ls.restate = lambda: None
    ls.step(32)
    assert np.array_equal(ls.a.state_digests(), ls.b.state_digests())
    sa, sb = ls.a.snapshot(), ls.b.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    ls.a.set_replay([])                                    # off: buffers freed, draining is refused
    with pytest.raises(ValueError):
        ls.a.drain_replay()
    ls.step(2)
    assert np.array_equal(ls.a.state_digests(), ls.b.state_digests())


def test_set_replay_refuses_bad_lists_and_host_buffers():
    prog, cm = build(small_lean())
    eng = BatchedMettaGrid(prog, np.repeat(cm[None], 4, 0), np.arange(4, dtype=np.uint32), buffers="device", specialize=False)
    for bad in ([0, 4], [-1], [1, 1]):
        with pytest.raises(ValueError):
            eng.set_replay(bad)
    with pytest.raises(ValueError):
        eng.set_replay([0], words_per_env=0)
    host = BatchedMettaGrid(prog, np.repeat(cm[None], 2, 0), np.arange(2, dtype=np.uint32), buffers="host", specialize=False)
    with pytest.raises(ValueError):
        host.set_replay([0])


# ---- (h) load / copy / reset onto a watched env ------------------------------------------------------------------------------
def test_load_copy_and_reset_onto_a_watched_env_cut_the_episode():
    prog, cm = build(small_lean())
    E = 4
    ls = Lockstep(prog, np.repeat(cm[None], E, 0), np.arange(E, dtype=np.uint32), [1, 2, 3])
    ls.step(3)
    saved_a, saved_b = ls.a.save_envs([0]), ls.b.save_envs([0])
    ls.step(2)

    def cut(k, flags):
        ls.want[k].append(rp.encode_end(ls.shadows[k], 5, flags))
    ls.a.load_envs(saved_a, [1]); ls.b.load_envs(saved_b, [1]); cut(0, K.RPL_E_DISCONTINUITY)
    ls.a.copy_envs([0], [2]); ls.b.copy_envs([0], [2]); cut(1, K.RPL_E_DISCONTINUITY)
    mask = np.array([0, 0, 0, 1], np.uint8)
    ls.a.reset_envs(mask); ls.b.reset_envs(mask); cut(2, K.RPL_E_ABORTED)
    ls.step(2)
    words, want, flags = ls.drain()
    for k, flag in enumerate((K.RPL_E_DISCONTINUITY, K.RPL_E_DISCONTINUITY, K.RPL_E_ABORTED)):
        assert np.array_equal(words[k], want[k])
        parsed = rp.parse_words(words[k])
        i = next(i for i, p in enumerate(parsed) if p[0] == "end")
        assert parsed[i][1] == flag and parsed[i][2] == 5 and parsed[i + 1][:2] == ("step", K.RPL_F_KEYFRAME)
    assert rp.parse_words(words[0])[-1][2] == 3 + 2      # env 1 goes on from the saved step 3


# ---- MettaGridBatchedEnv(replay_envs=..., replay_dir=...) ----------------------------------------------------------------------
def test_batched_env_writes_one_file_per_watched_episode(tmp_path):
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    prog, cm = build(small_lean(max_steps=8), ranks=(10, 11, 40, 41))
    env = MettaGridBatchedEnv(prog, 4, map_pool=np.stack([cm, cm]), episode_log=16, specialize=False, replay_envs=[1, 3],
                              replay_dir=str(tmp_path), replay_interval=8)
    env.reset(seed=5)
    rng = np.random.RandomState(3)
    n = env.transport_action_n
    for _ in range(17):
        env.step(torch.as_tensor(rng.randint(0, n, env.num_agents).astype(np.int32)).to(env.engine.obs.device))
    infos = env.episode_infos()
    with_path = [i for i in infos if "replay_path" in i]
    assert sorted((i["env"], i["episode"]) for i in with_path) == [(1, 0), (1, 1), (3, 0), (3, 1)]
    assert all(i["env"] in (1, 3) or "replay_path" not in i for i in infos)
    for i in with_path:
        doc = rp.read_replay(i["replay_path"])
        assert doc["infos"]["attributes"]["seed"] == i["attributes"]["seed"]      # the seed the device restarted the env with
        assert doc["version"] == 4 and doc["max_steps"] == 8 and doc["num_agents"] == 4 and len(doc["objects"]) > 4
        assert np.allclose(doc["infos"]["episode_rewards"], i["episode_rewards"], rtol=1e-5, atol=1e-5)   # f64 sum of f32 steps vs the engine's f32 sum
    env.close()
