"""GPU: the lean world kernel's batched per-agent passes in their wavefront-cooperative form (MgxDev::coop_passes,
csrc/mgx_world.h: a full wavefront walks the agents of its 32 envs as one flat run — clears, staging, the straight vibe pass,
tail_shadow_flat) against the per-env form they replace (MGX_WORLD_PASSES_PER_ENV) by state digest, and against the oracle
on crowded arenas with invalid action ids, at agent counts where an env's run of lanes straddles the 64-lane trips (6, 24:
p / A is a real division) and at env counts with full, partial and empty wavefronts."""
import dataclasses

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_class_maps, random_map

pytestmark = pytest.mark.gpu

SWITCH = "MGX_WORLD_PASSES_PER_ENV"


def test_cooperative_passes_equal_per_env_passes_by_digest(monkeypatch):
    """Rung-3 preset, 32x32, 200 envs = three full workgroups and one with a partial and an empty wavefront; 40 steps, primary
    ids from [-1, n_act] (invalid on both sides), vibe ids from [0, n_act).  Equal digests every 10 steps; equal observations,
    rewards, action_success and stats at the end.  Both engines keep the integer bookkeeping (tail_shadow is what runs)."""
    import torch
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    E, steps = 200, 40
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    seeds = np.arange(E, dtype=np.uint32)
    monkeypatch.delenv(SWITCH, raising=False)
    coop = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.setenv(SWITCH, "1")
    per_env = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(SWITCH)
    assert (coop.integer_bookkeeping, per_env.integer_bookkeeping) == (3, 3)
    assert (coop.act_variant, per_env.act_variant) == (0, 0)
    A, n_act = prog.num_agents, len(prog.action_names)
    gen = torch.Generator(device="cuda").manual_seed(11)
    for t in range(steps):
        a = torch.randint(-1, n_act + 1, (E * A,), dtype=torch.int32, device="cuda", generator=gen)
        v = torch.randint(0, n_act, (E * A,), dtype=torch.int32, device="cuda", generator=gen)
        for g in (coop, per_env):   # (the engines run on their own streams: order them behind the action writes and back)
            g.actions.copy_(a); g.vibe_actions.copy_(v)
            g.wait_for_caller(); g.step(); g.caller_waits()
        if t % 10 == 9:
            dc, dp = coop.state_digests(), per_env.state_digests()
            bad = np.nonzero(dc != dp)[0]
            assert len(bad) == 0, f"step {t + 1}: envs {bad[:8].tolist()} differ ({len(bad)})"
    torch.cuda.synchronize()
    assert torch.equal(coop.obs, per_env.obs) and torch.equal(coop.rewards, per_env.rewards)
    assert np.array_equal(coop.action_success(), per_env.action_success())
    assert np.array_equal(coop.executed_actions(), per_env.executed_actions())
    for i in range(E):
        for x, y in zip(coop.raw_stats(i), per_env.raw_stats(i)):
            assert np.array_equal(x, y), f"stats of env {i} differ"
    assert coop.poll_errors()[0] == 0 and per_env.poll_errors()[0] == 0
    coop.close(); per_env.close()


def _against_oracle(prog, cms, seeds, steps, rng_seed, where):
    import torch
    E, A = len(cms), prog.num_agents
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    assert eng.act_variant == 0 and eng.integer_bookkeeping == 3, (where, eng.act_variant, eng.integer_bookkeeping)
    oracles = [op.OracleSim(prog, cms[i], int(seeds[i])) for i in range(E)]
    for o in oracles:
        o.reinit_buffers()
    rng = np.random.default_rng(rng_seed)
    n_act = len(prog.action_names)
    for t in range(steps):
        a = rng.integers(-1, n_act + 1, E * A).astype(np.int32)
        v = rng.integers(-1, n_act + 1, E * A).astype(np.int32)   # (invalid ids in the vibe stream too: the marked entries)
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
    eng.close()


@pytest.mark.parametrize("per_team,E", [(8, 1), (8, 33), (8, 96), (3, 33), (12, 33)])
def test_cooperative_passes_against_oracle(per_team, E, monkeypatch):
    """Crowded 11x11 arenas (9x9 floor), 40 steps, ids from [-1, n_act] in both streams.  E = 1: a partial wavefront only (the
    per-env form); 33: one full wavefront and one partial; 96: a full workgroup and a full wavefront.  6 and 24 agents per
    env: 192 and 768 elements per wavefront, an env's agents spread over two lanes' trips."""
    monkeypatch.delenv(SWITCH, raising=False)
    # 24 agents and 9 objects on 81 floor cells show some agents more than the preset's 200 tokens; the reference raises there
    # and stops counting, so above 16 agents the rows get 400 tokens (the crowded 64-agent arena of test_gpu_act.py has 400 too)
    base = presets.rung3_spec(obs_tokens=200 if per_team <= 8 else 400)
    red, blue = base.agents[0], base.agents[-1]
    spec = dataclasses.replace(base, agents=[dataclasses.replace(red) for _ in range(per_team)] +
                               [dataclasses.replace(blue) for _ in range(per_team)])
    prog = compile_spec(spec, 11, 11, max_objects=192)
    assert prog.num_agents == 2 * per_team
    maps = [random_map(11, 11, {"wall": 3, "extractor": 4, "chest": 2}, {"red": per_team, "blue": per_team}, 700 + s) for s in range(E)]
    cms = np.stack([prog.class_map(m) for m in maps])
    _against_oracle(prog, cms, np.arange(E, dtype=np.uint32) + 13, 40, 3 + per_team, f"cooperative passes, {2 * per_team} agents")
