"""GPU: the lean world kernel's resolved move targets and run-ahead (MgxDev::move_fast, csrc/mgx_world.h: every agent's cell
ahead and its class's on_use are fetched in the staging pass, and the env's lane runs consecutive trivial actions of its order
without a load) against the general path they replace (MGX_NO_MOVE_FAST) by state digest, and against the oracle on crowded
arenas where resolved entries go stale: swaps displace agents, cells are vacated and entered earlier in the same tick."""
import copy
import dataclasses

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd import spec as S
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_class_maps, random_map

pytestmark = pytest.mark.gpu

SWITCH = "MGX_NO_MOVE_FAST"
COUNT = "MGX_MOVE_FAST_COUNT"


def _pair(prog, cms, seeds, monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setenv(COUNT, "1")
    fast = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.setenv(SWITCH, "1")
    slow = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(SWITCH)
    monkeypatch.delenv(COUNT)
    assert fast.move_fast != 0 and slow.move_fast == 0
    assert (fast.act_variant, slow.act_variant) == (0, 0) and (fast.dispatch_pairs, slow.dispatch_pairs) == (1, 1)
    return fast, slow


def _ab_by_digest(prog, cms, steps, seed, monkeypatch):
    """Same maps, seeds and action traces through both paths: equal digests every 10 steps; equal observations, rewards,
    action_success, executed actions and stats at the end.  Primary ids from [-1, n_act] (invalid on both sides)."""
    import torch
    E = len(cms)
    fast, slow = _pair(prog, cms, np.arange(E, dtype=np.uint32), monkeypatch)
    A, n_act = prog.num_agents, len(prog.action_names)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for t in range(steps):
        a = torch.randint(-1, n_act + 1, (E * A,), dtype=torch.int32, device="cuda", generator=gen)
        v = torch.randint(0, n_act, (E * A,), dtype=torch.int32, device="cuda", generator=gen)
        for g in (fast, slow):   # (the engines run on their own streams: order them behind the action writes and back)
            g.actions.copy_(a); g.vibe_actions.copy_(v)
            g.wait_for_caller(); g.step(); g.caller_waits()
        if t % 10 == 9:
            df, ds = fast.state_digests(), slow.state_digests()
            bad = np.nonzero(df != ds)[0]
            assert len(bad) == 0, f"step {t + 1}: envs {bad[:8].tolist()} differ ({len(bad)})"
    torch.cuda.synchronize()
    assert torch.equal(fast.obs, slow.obs) and torch.equal(fast.rewards, slow.rewards)
    assert np.array_equal(fast.action_success(), slow.action_success())
    assert np.array_equal(fast.executed_actions(), slow.executed_actions())
    for i in range(E):
        for x, y in zip(fast.raw_stats(i), slow.raw_stats(i)):
            assert np.array_equal(x, y), f"stats of env {i} differ"
    assert fast.poll_errors()[0] == 0 and slow.poll_errors()[0] == 0
    ran, stale = fast.move_fast_counts()
    assert slow.move_fast_counts() == (0, 0)
    fast.close(); slow.close()
    return ran, stale


@pytest.mark.parametrize("E", [200, 45])
def test_move_fast_equals_general_path_by_digest(E, monkeypatch):
    """Rung-3 preset, 32x32, 120 steps.  200 envs: three full workgroups, then a partial wavefront (8 envs: the per-env form of
    the resolve pass); 45: one full wavefront and one of 13 envs."""
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    ran, stale = _ab_by_digest(prog, cms, 120, 21, monkeypatch)
    # 13 of 15 ids are valid and 9 of those are noops or moves, nearly all of them trivial on a sparse map
    assert ran > E * prog.num_agents * 120 // 4, (ran, stale)


def test_hashed_dirty_set_on_a_large_map(monkeypatch):
    """40x40 = 1 600 cells: above 1 024 the dirty set is a 128-bit hashed mask.  Its false positives only send actions down
    the general path: equal digests, and both the run-ahead and the stale path are taken."""
    prog = compile_spec(presets.rung3_spec(), 40, 40, max_objects=256)
    E = 70
    cms = random_class_maps(prog, 40, 40, {"wall": 60, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    ran, stale = _ab_by_digest(prog, cms, 60, 23, monkeypatch)
    assert ran > 0 and stale > 0, (ran, stale)


def _against_oracle(prog, cms, seeds, steps, rng_seed, where, expect_fast):
    import torch
    E, A = len(cms), prog.num_agents
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    assert eng.act_variant == 0 and (eng.move_fast != 0) == expect_fast, (where, eng.act_variant, eng.move_fast)
    oracles = [op.OracleSim(prog, cms[i], int(seeds[i])) for i in range(E)]
    for o in oracles:
        o.reinit_buffers()
    rng = np.random.default_rng(rng_seed)
    n_act = len(prog.action_names)
    moves = np.array([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=np.int32)
    assert len(moves) == 8
    for t in range(steps):
        # two thirds moves (swaps with same-team neighbours, attacks, extractor and chest use, cells vacated or entered earlier
        # in the tick), the rest anything from [-1, n_act]: noops, wrong-stream ids, invalid ids on both sides
        a = rng.integers(-1, n_act + 1, E * A).astype(np.int32)
        mv = rng.random(E * A) < 2 / 3
        a[mv] = moves[rng.integers(0, len(moves), int(mv.sum()))]
        v = rng.integers(-1, n_act + 1, E * A).astype(np.int32)
        eng.actions.copy_(torch.from_numpy(a)); eng.vibe_actions.copy_(torch.from_numpy(v)); torch.cuda.synchronize()
        eng.step()
        snap = eng.snapshot()
        for i, o in enumerate(oracles):
            o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
            hp.compare_snapshots(o.snapshot(), {k: x[i * A:(i + 1) * A] for k, x in snap.items()}, f"{where} env {i} step {t + 1}")
    bits = 0
    for o in oracles:
        bits |= int(o.error)
    assert eng.poll_errors()[0] == bits     # (crowded arenas may overflow the token budget: both sides flag it)
    snap = eng.snapshot()
    for i, o in enumerate(oracles):
        mine = {k: x[i * A:(i + 1) * A] for k, x in snap.items()}
        pa = hp.payload_from_raw(prog, o.raw_objects(), o.current_stat_reward(), o.raw_stats(), o.snapshot(), steps, int(seeds[i]))
        pb = hp.payload_from_raw(prog, eng.raw_objects(i), eng.current_stat_reward(i), eng.raw_stats(i), mine, steps, int(seeds[i]))
        assert pa == pb, f"{where} env {i}: signature payload differs: {hp.diff_payload(pa, pb)}"
    counts = eng.move_fast_counts()
    eng.close()
    return counts


def _crowded(per_team, size, objs, E, seed0):
    # (24 agents in a small arena show some agents more than the preset's 200 tokens: 400 above 16 agents, like the other
    # crowded arenas of the suite)
    base = presets.rung3_spec(obs_tokens=200 if per_team <= 8 else 400)
    red, blue = base.agents[0], base.agents[-1]
    spec = dataclasses.replace(base, agents=[dataclasses.replace(red) for _ in range(per_team)] +
                               [dataclasses.replace(blue) for _ in range(per_team)])
    prog = compile_spec(spec, size, size, max_objects=192)
    assert prog.num_agents == 2 * per_team
    maps = [random_map(size, size, dict(objs), {"red": per_team, "blue": per_team}, seed0 + s) for s in range(E)]
    return prog, np.stack([prog.class_map(m) for m in maps])


@pytest.mark.parametrize("per_team,size,E", [(8, 11, 1), (8, 11, 33), (3, 9, 33), (12, 9, 33), (3, 13, 33), (12, 13, 33)])
def test_move_fast_against_oracle_on_crowded_arenas(per_team, size, E, monkeypatch):
    """16 agents on 11x11, 6 and 24 agents on 9x9 and 13x13; 60 steps.  E = 1 (the smallest case: a partial wavefront, the
    per-env resolve pass) and 33 (a full wavefront — the flat resolve pass — and a partial one).  The counters show that both
    the run-ahead and the stale-then-general path were taken."""
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setenv(COUNT, "1")
    objs = {"wall": 3, "extractor": 4, "chest": 2} if size > 9 else {"wall": 1, "extractor": 2, "chest": 1}
    prog, cms = _crowded(per_team, size, objs, E, 500 + 10 * per_team + size)
    ran, stale = _against_oracle(prog, cms, np.arange(E, dtype=np.uint32) + 17, 60, 5 + per_team + size,
                                 f"move_fast, {2 * per_team} agents on {size}x{size}", True)
    assert ran > 0 and stale > 0, (ran, stale)


def test_other_move_handler_tables_keep_the_general_path(monkeypatch):
    """A custom move handler in front of the default pair (a ranged use: MaxDistance 2) is not the canonical table: move_fast
    reports 0 and the program runs as before, against the oracle."""
    monkeypatch.delenv(SWITCH, raising=False)
    spec = copy.deepcopy(presets.rung3_spec())
    spec.move_handlers = [S.Handler([S.VibeFilter(S.ACTOR, "b"), S.MaxDistanceFilter(S.TARGET, 2), S.TargetIsUsableFilter()],
                                    [S.UseTarget()], "reach")]
    prog = compile_spec(spec, 11, 11, max_objects=192)
    E = 8
    maps = [random_map(11, 11, {"wall": 3, "extractor": 4, "chest": 2}, {"red": 8, "blue": 8}, 820 + s) for s in range(E)]
    cms = np.stack([prog.class_map(m) for m in maps])
    counts = _against_oracle(prog, cms, np.arange(E, dtype=np.uint32) + 3, 30, 12, "ranged use in front of the default move", False)
    assert counts == (0, 0)
