"""GPU: chosen stats of every env and agent read out on the device behind every step (include/mgx.h mgx_set_step_stats,
csrc/mgx_step_stats.h) — the per-step info payload of MettaGridPufferEnv(step_info_keys=...)
(python/src/mettagrid/envs/mettagrid_puffer_env.py:132-183, 230-282).  After EVERY step the tensors are compared bit for bit,
values and "key exists" flags, with the oracle's stats of all envs; no mgx_get_stats / mgx_state_digests call (each runs the
flush of the integer bookkeeping, which would hide a stale stat cell) comes before the comparison is over."""
import numpy as np
import pytest

import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv, decode_actions
from mettagrid_amd.fmt import K
from mettagrid_amd.mapgen import random_class_maps

pytestmark = pytest.mark.gpu

COUNTERS = ("action.move.success", "action.failed", "status.max_steps_without_motion")
COVERAGE = ("cell.unique_visited", "cell.max_distance_from_spawn")
AGENT_KEYS = COUNTERS + COVERAGE + ("ore.gained", "reward_step", "reward_episode", "no.such.stat")
AGENT_KEYS_5 = ("action.move.success", "status.max_steps_without_motion", "cell.unique_visited", "reward_step", "no.such.stat")
GAME_KEYS = ("objects.wall", "tokens_written", "attributes/steps")


def _rung3(E):   # (as tests/test_gpu_bookkeeping.py builds it)
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    return prog, cms


def _rung4(E):
    prog = compile_spec(presets.rung4_spec(max_steps=0), 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
    cms = np.stack([prog.class_map(presets.rung4_map(50 + m)) for m in range(E)])
    return prog, cms


def _expected(prog, oracle, game_keys, agent_keys):
    """What the tensors' rows of one env must hold, from the oracle: (game f32 [KG], exists u8 [KG], agent f32 [A, KA], exists)."""
    gv, gt, av, at = oracle.raw_stats()
    snap = oracle.snapshot()
    A = prog.num_agents
    gid = {n: i for i, n in enumerate(prog.game_stat_names)}
    aid = {n: i for i, n in enumerate(prog.agent_stat_names)}
    g, ge = np.zeros(len(game_keys), np.float32), np.zeros(len(game_keys), np.uint8)
    for c, k in enumerate(game_keys):
        if k == "attributes/steps":
            g[c], ge[c] = np.float32(oracle.current_step), 1
        elif k in gid:
            g[c], ge[c] = gv[gid[k]], gt[gid[k]]
    a, ae = np.zeros((A, len(agent_keys)), np.float32), np.zeros((A, len(agent_keys)), np.uint8)
    for c, k in enumerate(agent_keys):
        if k == "reward_step":
            a[:, c], ae[:, c] = snap["rewards"], 1
        elif k == "reward_episode":
            a[:, c], ae[:, c] = snap["episode_rewards"], 1
        elif k in aid:
            a[:, c], ae[:, c] = av[:, aid[k]], at[:, aid[k]]
    return g, ge, a, ae


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _count_flushing_reads(monkeypatch):
    """Counts the engine calls that flush the integer bookkeeping into the stat rows."""
    calls = []
    for name in ("raw_stats", "state_digests"):
        orig = getattr(BatchedMettaGrid, name)
        monkeypatch.setattr(BatchedMettaGrid, name, lambda self, *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(self, *a, **kw))[1])
    return calls


def _compare_with_oracle(monkeypatch, prog, cms, agent_keys, steps=40, want_mode=None, rng_seed=3):
    import torch
    calls = _count_flushing_reads(monkeypatch)
    E, A = len(cms), prog.num_agents
    seeds = np.arange(E, dtype=np.uint32) * 5 + 17
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="device")
    mode = eng.integer_bookkeeping
    if want_mode is not None:
        assert mode == want_mode, mode
    eng.set_step_stats(GAME_KEYS, agent_keys)
    gk, ak = eng.step_stats_columns()
    assert gk == ["stat" if k in prog.game_stat_names else "absent" for k in GAME_KEYS[:-1]] + ["steps"]
    for k, kind in zip(agent_keys, ak):   # a column is an integer kind exactly in an engine that keeps that stat as an integer
        want = ("counter" if k in COUNTERS and mode & 1 else "cov_unique" if k == COVERAGE[0] and mode & 2 else
                "cov_maxdist" if k == COVERAGE[1] and mode & 2 else k if k.startswith("reward_") else
                "stat" if k in prog.agent_stat_names else "absent")
        assert kind == want, (k, kind, want, mode)
    oracles = [op.OracleSim(prog, cms[i], int(seeds[i])) for i in range(E)]
    for o in oracles:
        o.reinit_buffers()
    rng = np.random.default_rng(rng_seed)
    n_act = len(prog.action_names)
    tg, tge, ta, tae = eng.step_stats
    assert tuple(tg.shape) == (E, len(GAME_KEYS)) and tuple(ta.shape) == (E * A, len(agent_keys))
    for t in range(steps):
        a = rng.integers(-1, n_act + 1, E * A).astype(np.int32)   # invalid ids on both sides of the table included
        v = rng.integers(0, n_act, E * A).astype(np.int32)
        eng.actions.copy_(torch.from_numpy(a)); eng.vibe_actions.copy_(torch.from_numpy(v)); torch.cuda.synchronize()
        eng.step()
        eng.sync()
        g, ge, ag, age = tg.cpu().numpy(), tge.cpu().numpy(), ta.cpu().numpy(), tae.cpu().numpy()
        for i, o in enumerate(oracles):
            o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
            xg, xge, xa, xae = _expected(prog, o, GAME_KEYS, agent_keys)
            where = f"env {i} step {t + 1}"
            assert np.array_equal(ge[i], xge), (where, GAME_KEYS, ge[i], xge)
            assert np.array_equal(_bits(g[i]), _bits(xg)), (where, GAME_KEYS, g[i], xg)
            assert np.array_equal(age[i * A:(i + 1) * A], xae), (where, agent_keys, age[i * A:(i + 1) * A], xae)
            assert np.array_equal(_bits(ag[i * A:(i + 1) * A]), _bits(xa)), (where, agent_keys, ag[i * A:(i + 1) * A], xa)
    assert calls == [], calls   # nothing flushed the counters into the stat rows while the comparison ran
    assert eng.poll_errors()[0] == 0
    return eng, (g, ge, ag, age)


@pytest.mark.parametrize("agent_keys", [AGENT_KEYS, AGENT_KEYS_5], ids=["all_keys", "five_keys"])
def test_every_step_matches_the_oracle(monkeypatch, agent_keys):
    """70 envs x 16 agents = 1 120 rows; with 9 (5) agent columns and 3 game columns the pair count 10 290 (5 810) is no
    multiple of the wavefront or the workgroup, and the kernel runs more than one workgroup.  Then the existing read path:
    mgx_get_stats of three envs holds what the tensors' rows hold."""
    prog, cms = _rung3(70)
    eng, (g, ge, ag, age) = _compare_with_oracle(monkeypatch, prog, cms, agent_keys, want_mode=3)
    A = prog.num_agents
    aid = {n: i for i, n in enumerate(prog.agent_stat_names)}
    for i in (0, 33, 69):
        gv, gt, av, at = eng.raw_stats(i)
        for c, k in enumerate(GAME_KEYS[:-1]):
            j = prog.game_stat_names.index(k)
            assert _bits(g[i, c]) == _bits(gv[j]) and ge[i, c] == gt[j], (i, k)
        for c, k in enumerate(agent_keys):
            if k in aid:
                assert np.array_equal(_bits(ag[i * A:(i + 1) * A, c]), _bits(av[:, aid[k]])), (i, k)
                assert np.array_equal(age[i * A:(i + 1) * A, c], at[:, aid[k]]), (i, k)
    eng.close()


@pytest.mark.parametrize("switch, mode", [("MGX_ACT_LEAN", 1), ("MGX_NO_SHADOW", 0)])
def test_other_bookkeeping_modes(monkeypatch, switch, mode):
    """Mode 1 (lane-per-agent dispatch): counters integer, coverage stats in the rows; mode 0: everything in the rows."""
    monkeypatch.setenv(switch, "1")
    prog, cms = _rung3(6)
    eng, _ = _compare_with_oracle(monkeypatch, prog, cms, AGENT_KEYS, want_mode=mode)
    eng.close()


def test_extended_game(monkeypatch):
    prog, cms = _rung4(3)
    eng, _ = _compare_with_oracle(monkeypatch, prog, cms, AGENT_KEYS)
    eng.close()


def _step_both(engs, prog, E, steps, rng_seed):
    import torch
    A, n_act = prog.num_agents, len(prog.action_names)
    rng = np.random.default_rng(rng_seed)
    for t in range(steps):
        a = rng.integers(-1, n_act + 1, E * A).astype(np.int32)
        v = rng.integers(0, n_act, E * A).astype(np.int32)
        for eng in engs:
            eng.actions.copy_(torch.from_numpy(a)); eng.vibe_actions.copy_(torch.from_numpy(v))
        torch.cuda.synchronize()
        for eng in engs:
            eng.step()
        for eng in engs:
            eng.sync()


def test_the_readout_changes_no_engine_state():
    E = 16
    prog, cms = _rung3(E)
    seeds = np.arange(E, dtype=np.uint32) + 4
    with_keys, without = (BatchedMettaGrid(prog, cms, seeds, buffers="device") for _ in range(2))
    with_keys.set_step_stats(GAME_KEYS, AGENT_KEYS)
    assert without.step_stats is None
    _step_both((with_keys, without), prog, E, 40, 8)
    assert np.array_equal(with_keys.state_digests(), without.state_digests())
    assert np.array_equal(with_keys.obs.cpu().numpy(), without.obs.cpu().numpy())
    with_keys.close(); without.close()


def test_off_switch_leaves_the_tensors_alone():
    import torch
    E = 5
    prog, cms = _rung3(E)
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device")
    eng.set_step_stats(GAME_KEYS, AGENT_KEYS)
    _step_both((eng,), prog, E, 3, 1)
    tensors = eng.step_stats
    assert float(tensors[0][:, 2].min()) == 3.0 and int(tensors[3][:, 6].min()) == 1   # attributes/steps, reward_step exists
    eng.set_step_stats([], [])
    assert eng.step_stats is None
    for t in tensors:
        t.fill_(77)
    torch.cuda.synchronize()
    _step_both((eng,), prog, E, 2, 2)
    for t in tensors:
        assert bool((t == 77).all())
    eng.set_step_stats(["attributes/steps"], [])   # ... and on again, game columns only
    _step_both((eng,), prog, E, 1, 3)
    assert eng.step_stats[0].cpu().numpy().tolist() == [[6.0]] * E and tuple(eng.step_stats[2].shape) == (E * prog.num_agents, 0)
    eng.close()


def test_refusals():
    import ctypes as C
    import torch
    E = 2
    prog, cms = _rung3(E)
    A, NG, NS = prog.num_agents, len(prog.game_stat_names), len(prog.agent_stat_names)
    out = (torch.zeros((E, 65), dtype=torch.float32, device="cuda"), torch.zeros((E, 65), dtype=torch.uint8, device="cuda"),
           torch.zeros((E * A, 65), dtype=torch.float32, device="cuda"), torch.zeros((E * A, 65), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    ptrs = [C.c_void_p(t.data_ptr()) for t in out]

    def call(eng, g, a, p=ptrs):
        g, a = np.asarray(g, dtype=np.int32), np.asarray(a, dtype=np.int32)
        return eng.L.mgx_set_step_stats(eng.h, g.ctypes.data if g.size else None, int(g.size), a.ctypes.data if a.size else None,
                                        int(a.size), *p)

    host = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="host")
    assert call(host, [0], [0]) == -1 and b"MGX_MEM_HOST" in host.L.mgx_last_error()
    with pytest.raises(ValueError, match="host buffers"):
        host.set_step_stats(GAME_KEYS, AGENT_KEYS)
    assert call(host, [], []) == 0   # (off is always accepted)
    host.close()

    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device")
    assert call(eng, [0] * 65, [0]) == -1 and call(eng, [0], [0] * 65) == -1 and b"at most 64" in eng.L.mgx_last_error()
    assert call(eng, [NG], [0]) == -1 and call(eng, [0], [NS]) == -1 and b"agent column 0: id" in eng.L.mgx_last_error()
    assert call(eng, [-5], []) == -1 and call(eng, [], [-5]) == -1
    assert call(eng, [K.SS_REWARD_STEP], []) == -1 and call(eng, [], [K.SS_STEPS]) == -1   # a code of the other table
    assert call(eng, [0], [], [None, ptrs[1], ptrs[2], ptrs[3]]) == -1 and call(eng, [], [0], [ptrs[0], ptrs[1], ptrs[2], None]) == -1
    assert eng.L.mgx_step_stats_columns(eng.h, np.zeros(4, np.int32).ctypes.data) == -1   # nothing was accepted: nothing is set
    with pytest.raises(ValueError, match="at most 64"):
        eng.set_step_stats(["objects.wall"] * 65, [])
    assert call(eng, [0] * 64, [0] * 64) == 0   # the limit itself is fine
    _step_both((eng,), prog, E, 1, 0)
    g64 = out[0].flatten()[:E * 64].view(E, 64)   # (the engine's row pitch is the column count it was given)
    assert bool((g64 == g64[:, :1]).all()) and bool((out[1].flatten()[:E * 64] == 1).all()) and eng.poll_errors()[0] == 0
    assert call(eng, [NG], [0]) == -1           # a refused call leaves the running readout as it is
    kinds = np.zeros(128, np.int32)
    assert eng.L.mgx_step_stats_columns(eng.h, kinds.ctypes.data) == 0 and kinds[0] == K.SSK_STAT
    eng.close()


def _reference_payload(prog, oracle, keys, seed):
    """_build_step_info_payload (mettagrid_puffer_env.py:230-282) restated over the oracle, without the episode-end infos."""
    gv, gt, av, at = oracle.raw_stats()
    snap = oracle.snapshot()
    words = prog.words
    gid = {n: i for i, n in enumerate(prog.game_stat_names)}
    aid = {n: i for i, n in enumerate(prog.agent_stat_names)}
    game_keys, attr_keys, agent_keys = keys
    out = {}
    for raw, stat in game_keys:
        if stat in gid and gt[gid[stat]]:
            out[raw] = float(gv[gid[stat]])
    attrs = {"seed": float(seed), "map_w": float(words[4]), "map_h": float(words[3]), "steps": float(oracle.current_step),
             "max_steps": float(words[11])}
    for raw, attr in attr_keys:
        out[raw] = attrs[attr]
    per = {}
    for i in range(prog.num_agents):
        row = {}
        for k in agent_keys:
            if k == "reward_step":
                row[k] = float(snap["rewards"][i])
            elif k == "reward_episode":
                row[k] = float(snap["episode_rewards"][i])
            elif k in aid and at[i, aid[k]]:
                row[k] = float(av[i, aid[k]])
        per[i] = row
    out["_per_agent_infos"] = per
    return out


def test_auto_reset_reports_the_finished_episode_then_the_new_one():
    """MettaGridBatchedEnv(step_info_keys=...) over a 4-map pool, 11-step episodes: the step that truncates an env reports
    steps = 11 and the finished episode's counters, the step after it steps = 1 — when the reference builds those payloads."""
    import torch
    from mettagrid_amd.envs import parse_step_info_keys
    spec = presets.rung3_spec()
    spec.max_steps = 11
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    E, A, M = 8, prog.num_agents, 4
    pool = np.stack([prog.class_map(presets.rung3_map(50 + m)) for m in range(M)])
    keys = ["game/objects.wall", "env_game/tokens_written", "team/red/no.such.stat", "attributes/steps", "env_attributes/seed",
            "attributes/max_steps", "attributes/map_w", "attributes/map_h", "game/objects.wall"] + ["agent/" + k for k in AGENT_KEYS]
    plain = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=5, validate_actions=False)
    plain.reset()
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=5, validate_actions=False, step_info_keys=keys)
    _, infos = env.reset()
    assert infos == {}
    parsed = parse_step_info_keys(keys)
    seeds = env._seeds()
    oracles = [op.OracleSim(prog, pool[e % M], int(seeds[e])) for e in range(E)]
    for o in oracles:
        o.reinit_buffers()
    episode, ended = [0] * E, [False] * E
    n_primary, vibe_ids = len(env.action_names), np.asarray(env._vibe_ids_host, dtype=np.int64)
    rng = np.random.default_rng(9)
    steps_col = env._si_game_columns.index("attributes/steps")
    move_col = AGENT_KEYS.index("action.move.success")
    saw_end = saw_restart = 0
    for t in range(30):
        for e in range(E):
            if ended[e]:   # the reference wrapper builds the new Simulation at the start of the next step (:299-302)
                episode[e] += 1
                oracles[e] = op.OracleSim(prog, pool[(e + episode[e]) % M], int(seeds[e]))
                oracles[e].reinit_buffers()
        a = rng.integers(0, env.transport_action_n, E * A).astype(np.int32)
        core, vibe = decode_actions(a, n_primary, vibe_ids)
        vibe = np.zeros(E * A, np.int64) if vibe is None else vibe
        *_, infos = env.step(torch.from_numpy(a).cuda())
        if t < 3:   # without keys the step returns no such entry
            assert "step_info" not in plain.step(torch.from_numpy(a).cuda())[-1]
        si = infos["step_info"]
        assert si.game_keys == parsed[0] and si.attribute_keys == parsed[1] and si.agent_keys == parsed[2]
        env.engine.sync()
        steps_now = si.game[:, steps_col].cpu().numpy()
        moves = si.agent[:, move_col].cpu().numpy().reshape(E, A)
        for e, o in enumerate(oracles):
            was_ended = ended[e]
            o.step(core[e * A:(e + 1) * A], vibe[e * A:(e + 1) * A])
            ended[e] = bool(o.snapshot()["truncations"].all())
            assert si.payload(e) == _reference_payload(prog, o, parsed, seeds[e]), (e, t)
            if ended[e]:
                assert steps_now[e] == 11.0 and o.current_step == 11
                assert np.array_equal(moves[e], o.raw_stats()[2][:, prog.agent_stat_names.index("action.move.success")])
                saw_end += 1
            if was_ended:
                assert steps_now[e] == 1.0
                saw_restart += 1
    assert saw_end == 2 * E and saw_restart == 2 * E
    env.close(); plain.close()
