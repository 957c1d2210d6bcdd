"""GPU: the lean world kernel's instance compiled for the rung-3 preset's shape (MgxWorldShapeR3, csrc/mgx_world.h: every
scalar of the engine's table a compile-time constant) — when the engine chooses it (`world_variant`), and that it computes
what the generic kernel (MGX_WORLD_GENERIC=1) and the oracle compute.  The instance exists at one shape only (32x32, 16
agents, 192 object slots), so that is the shape of every case here; the env counts are small."""
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

GENERIC = "MGX_WORLD_GENERIC"
OBJS = {"wall": 40, "extractor": 8, "chest": 4}
TEAMS = {"red": 8, "blue": 8}


def _preset(E):
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    return prog, random_class_maps(prog, 32, 32, OBJS, TEAMS, range(E))


def _engine(prog, cms, monkeypatch, **env):
    for k in (GENERIC, "MGX_NO_GEN", "MGX_NO_MOVE_FAST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return BatchedMettaGrid(prog, cms, np.arange(len(cms), dtype=np.uint32), buffers="device", specialize=False)
    finally:
        for k in env:
            monkeypatch.delenv(k)


# ---- selection ------------------------------------------------------------------------------------------------------------
def test_the_preset_takes_the_instance_and_the_switches_take_it_away(monkeypatch):
    prog, cms = _preset(4)
    for env, want, gen in (({}, 3, 3), ({GENERIC: "1"}, 0, 3), ({"MGX_NO_GEN": "1"}, 0, 0)):
        eng = _engine(prog, cms, monkeypatch, **env)
        try:
            assert (eng.world_variant, eng.handler_variant) == (want, gen), (env, eng.world_variant, eng.handler_variant)
            assert eng.obs_variant == 3 and eng.act_variant == 0
        finally:
            eng.close()


def _against_oracle(prog, cms, steps, rng_seed, where, monkeypatch, want_variant, **env):
    """Every env, every step from construction, against the oracle (observations, rewards, terminals, action_success; the
    signature payload at the end).  Two thirds moves, the rest from [-1, n_act]: invalid ids in both streams."""
    import torch
    E, A = len(cms), prog.num_agents
    eng = _engine(prog, cms, monkeypatch, **env)
    try:
        assert eng.world_variant == want_variant, (where, eng.world_variant)
        oracles = [op.OracleSim(prog, cms[i], i) for i in range(E)]
        for o in oracles:
            o.reinit_buffers()
        rng = np.random.default_rng(rng_seed)
        n_act = len(prog.action_names)
        moves = np.array([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=np.int32)
        for t in range(steps):
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
        assert eng.poll_errors()[0] == bits
        snap = eng.snapshot()
        for i, o in enumerate(oracles):
            mine = {k: x[i * A:(i + 1) * A] for k, x in snap.items()}
            pa = hp.payload_from_raw(prog, o.raw_objects(), o.current_stat_reward(), o.raw_stats(), o.snapshot(), steps, i)
            pb = hp.payload_from_raw(prog, eng.raw_objects(i), eng.current_stat_reward(i), eng.raw_stats(i), mine, steps, i)
            assert pa == pb, f"{where} env {i}: signature payload differs: {hp.diff_payload(pa, pb)}"
    finally:
        eng.close()


def _one_field_off(name):
    """The preset with ONE field of the shape changed: (program, class maps)."""
    spec, h, w, slots, teams, objs = copy.deepcopy(presets.rung3_spec()), 32, 32, 192, dict(TEAMS), dict(OBJS)
    if name == "31x32 map":
        h = 31
    elif name == "15 agents":
        spec = dataclasses.replace(spec, agents=spec.agents[:-1])
        teams = {"red": 8, "blue": 7}
    elif name == "191 slots":
        slots = 191
        objs["wall"] -= 1   # (the preset's maps fill all 192 slots: 124 border walls, 52 objects, 16 agents)
    elif name == "one action removed":
        spec = dataclasses.replace(spec, move_directions=spec.move_directions[:-1])
    elif name == "ranged move handler":
        spec.move_handlers = [S.Handler([S.VibeFilter(S.ACTOR, "b"), S.MaxDistanceFilter(S.TARGET, 2), S.TargetIsUsableFilter()],
                                        [S.UseTarget()], "reach")]
    prog = compile_spec(spec, h, w, max_objects=slots)
    maps = [random_map(h, w, objs, teams, 900 + s) for s in range(3)]
    return prog, np.stack([prog.class_map(m) for m in maps])


@pytest.mark.parametrize("name", ["31x32 map", "15 agents", "191 slots", "one action removed", "ranged move handler"])
def test_one_field_off_goes_to_the_generic_kernel(name, monkeypatch):
    """A program that differs from the preset in one field of the shape runs the generic kernel, with the results it had:
    against the oracle, 3 envs x 12 steps."""
    ref = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    prog, cms = _one_field_off(name)
    differs = {"31x32 map": cms.shape[1:] == (31, 32), "15 agents": prog.num_agents == ref.num_agents - 1,
               "191 slots": prog.max_objects == ref.max_objects - 1,
               "one action removed": len(prog.action_names) == len(ref.action_names) - 1, "ranged move handler": True}[name]
    assert differs, name
    _against_oracle(prog, cms, 12, 31, name, monkeypatch, 0)
    if name == "ranged move handler":
        eng = _engine(prog, cms, monkeypatch)
        try:
            assert eng.move_fast == 0
        finally:
            eng.close()


# ---- the instance against the generic kernel --------------------------------------------------------------------------------
def _ab_every_step(prog, cms, steps, seed, monkeypatch, first=None, other=None):
    """The preset's instance and the generic kernel (`other`: MGX_WORLD_GENERIC=1) side by side on the same maps, seeds and actions:
    equal state digests, observations, rewards, terminals, action_success, executed actions and stats after EVERY step.
    Two thirds moves; the rest from [-1, n_act] in both streams (invalid ids on both sides)."""
    import torch
    E, A, n_act = len(cms), prog.num_agents, len(prog.action_names)
    other = other or {GENERIC: "1"}
    inst = _engine(prog, cms, monkeypatch)
    gen = _engine(prog, cms, monkeypatch, **other)
    try:
        assert (inst.world_variant, gen.world_variant) == (3, 0)
        assert inst.move_fast != 0 and (gen.move_fast != 0) == ("MGX_NO_MOVE_FAST" not in other)
        g = torch.Generator(device="cuda").manual_seed(seed)
        moves = torch.tensor([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=torch.int32, device="cuda")
        for t in range(steps):
            a = torch.randint(-1, n_act + 1, (E * A,), dtype=torch.int32, device="cuda", generator=g)
            mv = torch.rand(E * A, device="cuda", generator=g) < 2 / 3
            pick = moves[torch.randint(0, len(moves), (E * A,), device="cuda", generator=g)]
            a = torch.where(mv, pick, a)
            v = torch.randint(-1, n_act + 1, (E * A,), dtype=torch.int32, device="cuda", generator=g)
            for e in (inst, gen):   # (the engines run on their own streams: order them behind the action writes and back)
                e.actions.copy_(a); e.vibe_actions.copy_(v)
                e.wait_for_caller(); e.step(); e.caller_waits()
            where = f"step {t + 1}"
            bad = np.nonzero(inst.state_digests() != gen.state_digests())[0]
            assert len(bad) == 0, f"{where}: digests of envs {bad[:8].tolist()} differ ({len(bad)})"
            torch.cuda.synchronize()
            assert torch.equal(inst.obs, gen.obs), where
            assert torch.equal(inst.rewards, gen.rewards) and torch.equal(inst.terminals, gen.terminals), where
            assert np.array_equal(inst.action_success(), gen.action_success()), where
            assert np.array_equal(inst.executed_actions(), gen.executed_actions()), where
            for i in range(E):
                for x, y in zip(inst.raw_stats(i), gen.raw_stats(i)):
                    assert np.array_equal(x, y), f"{where}: stats of env {i} differ"
        assert inst.poll_errors()[0] == 0 and gen.poll_errors()[0] == 0
    finally:
        inst.close(); gen.close()
        if first is not None:
            first.close()


@pytest.mark.parametrize("E", [200, 45])
def test_instance_equals_generic_kernel_every_step(E, monkeypatch):
    """120 steps.  200 envs: full wavefronts (the flat, wavefront-cooperative form of the batched passes) and a last one of
    8 envs; 45: one full wavefront and one of 13 envs (the per-env form)."""
    prog, cms = _preset(E)
    _ab_every_step(prog, cms, 120, 41, monkeypatch)


def test_instance_equals_generic_kernel_without_move_fast(monkeypatch):
    """The 200-env case with MGX_NO_MOVE_FAST=1.  The switch changes fields of the shape (move_fast and the LDS behind it), so
    an engine created under it runs the generic kernel on the general path of every move; the instance (run-ahead on) must
    agree with it after every step."""
    prog, cms = _preset(200)
    _ab_every_step(prog, cms, 120, 41, monkeypatch, other={"MGX_NO_MOVE_FAST": "1"})


def test_instance_on_the_other_constant_slot(monkeypatch):
    """Engines take the two constant-memory slots of the lean unit in turn.  With one more lean engine alive in front, the
    instance runs from the slot the generic kernel had in the cases above, and the other way round."""
    prog, cms = _preset(200)
    first = _engine(prog, cms[:2], monkeypatch)
    _ab_every_step(prog, cms, 120, 43, monkeypatch, first=first)


def test_instance_against_the_oracle(monkeypatch):
    prog, cms = _preset(16)
    _against_oracle(prog, cms, 40, 7, "preset instance", monkeypatch, 3)
