"""GPU: the pipelined run-ahead of the lean world kernel (csrc/mgx_world.h: the env's lane holds the next agent's record while it
processes this one, leaves one outcome byte per consumed agent, and a flat pass behind the primary stream writes the rest of
handle_action's bookkeeping) against the run-ahead's first form on the same binary (MGX_MF_SERIAL_BOOK=1: one agent at a time,
bookkeeping inside the loop), and that form against no run-ahead at all (MGX_NO_MOVE_FAST=1) — after EVERY step: state digest,
observations, rewards, terminals, action_success, executed actions and the run-ahead counters; every stat after every tenth step.
The crowded arenas are checked against the oracle too."""
import dataclasses

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import ascii_map, random_class_maps, random_map

pytestmark = pytest.mark.gpu

SERIAL = "MGX_MF_SERIAL_BOOK"
NO_MF = "MGX_NO_MOVE_FAST"
COUNT = "MGX_MOVE_FAST_COUNT"


def _trio(prog, cms, seeds, monkeypatch, preset=False):
    """The default engine, one with the serial run-ahead, one without run-ahead; all count.  preset: the default engine must be
    on the instance compiled for the preset's shape — the one that holds the pipelined loop only and that the benchmark runs."""
    for k in (SERIAL, NO_MF):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(COUNT, "1")
    new = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.setenv(SERIAL, "1")
    serial = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(SERIAL)
    monkeypatch.setenv(NO_MF, "1")
    slow = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(NO_MF)
    monkeypatch.delenv(COUNT)
    assert new.move_fast in (1, 3) and serial.move_fast == new.move_fast | 4 and slow.move_fast == 0
    assert serial.world_variant == 0 and slow.world_variant == 0   # the switches change fields of the shape: never the preset's instance
    assert new.world_variant == (3 if preset else 0), new.world_variant
    assert all(g.act_variant == 0 and g.dispatch_pairs == 1 for g in (new, serial, slow))
    return new, serial, slow


def _same(x, y, what):
    import torch
    ok = torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y)
    assert ok, what


def _same_stats(engines, E, where):
    for i in range(E):
        stats = [g.raw_stats(i) for g in engines]
        for other in stats[1:]:
            for x, y in zip(stats[0], other):
                assert np.array_equal(x, y), f"{where}: stats of env {i} differ"


def _run_trio(prog, cms, actions, monkeypatch, seeds=None, preset=False):
    """actions: a list of (primary, vibe) int32 arrays [E * A], one pair per step.  Returns the (ran, stale) counters.  The
    run-ahead counters are compared after every step, every agent and game stat after every tenth and after the last."""
    import torch
    E = len(cms)
    engines = _trio(prog, cms, np.arange(E, dtype=np.uint32) + 5 if seeds is None else seeds, monkeypatch, preset)
    new, serial, slow = engines
    for t, (a, v) in enumerate(actions):
        a, v = torch.from_numpy(a).cuda(), torch.from_numpy(v).cuda()
        for g in engines:   # (the engines run on their own streams: order them behind the action writes and back)
            g.actions.copy_(a); g.vibe_actions.copy_(v)
            g.wait_for_caller(); g.step(); g.caller_waits()
        torch.cuda.synchronize()
        for x, y, names in ((new, serial, "pipelined vs serial run-ahead"), (serial, slow, "serial run-ahead vs none")):
            where = f"{names}, step {t + 1}"
            dx, dy = x.state_digests(), y.state_digests()
            assert np.array_equal(dx, dy), f"{where}: envs {np.nonzero(dx != dy)[0][:8].tolist()} differ by digest"
            _same(x.obs, y.obs, f"{where}: observations")
            _same(x.rewards, y.rewards, f"{where}: rewards")
            _same(x.terminals, y.terminals, f"{where}: terminals")
            _same(x.action_success(), y.action_success(), f"{where}: action_success")
            _same(x.executed_actions(), y.executed_actions(), f"{where}: executed actions")
        assert new.move_fast_counts() == serial.move_fast_counts(), f"step {t + 1}: run-ahead counters"
        if t % 10 == 9:
            _same_stats(engines, E, f"step {t + 1}")
    _same_stats(engines, E, "last step")
    errs = [g.poll_errors()[0] for g in engines]
    assert errs[0] == errs[1] == errs[2], errs
    counts = new.move_fast_counts()
    assert serial.move_fast_counts() == counts and slow.move_fast_counts() == (0, 0)
    for g in engines:
        g.close()
    return counts, errs[0]


def _mixed_actions(prog, E, steps, seed, move_share=2 / 3):
    rng = np.random.default_rng(seed)
    A, n_act = prog.num_agents, len(prog.action_names)
    moves = np.array([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=np.int32)
    out = []
    for _ in range(steps):
        a = rng.integers(-1, n_act + 1, E * A).astype(np.int32)   # noops, wrong-stream ids, invalid ids on both sides
        mv = rng.random(E * A) < move_share
        a[mv] = moves[rng.integers(0, len(moves), int(mv.sum()))]
        out.append((a, rng.integers(-1, n_act + 1, E * A).astype(np.int32)))
    return out


def _rung3(size=32, slots=192):
    return compile_spec(presets.rung3_spec(), size, size, max_objects=slots)


def _rung3_maps(prog, E, size=32, walls=40):
    return random_class_maps(prog, size, size, {"wall": walls, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))


@pytest.mark.parametrize("E", [45, 200])
def test_preset_shape_two_thirds_moves(E, monkeypatch):
    """Rung-3 rules, 32x32, 16 agents, 120 steps: the preset's instance runs the pipelined loop.  45 envs: one full wavefront and
    one of 13 envs (the flat pass's per-env form and the clamp of the last positions); 200: three workgroups and 8 envs."""
    prog = _rung3()
    (ran, stale), err = _run_trio(prog, _rung3_maps(prog, E), _mixed_actions(prog, E, 120, 31 + E), monkeypatch, preset=True)
    assert err == 0 and ran > E * prog.num_agents * 120 // 4 and stale > 0, (ran, stale)


def _crowded(per_team, size, objs, E, seed0):
    base = presets.rung3_spec(obs_tokens=200 if per_team <= 8 else 400)
    red, blue = base.agents[0], base.agents[-1]
    spec = dataclasses.replace(base, agents=[dataclasses.replace(red) for _ in range(per_team)] +
                               [dataclasses.replace(blue) for _ in range(per_team)])
    prog = compile_spec(spec, size, size, max_objects=192)
    if objs == "ring":   # the agents on the inner cells, every cell around them an extractor or a chest: most moves meet an on_use
        maps = []
        for s in range(E):
            m = random_map(size, size, {}, 0, 0)
            m[1:-1, 1:-1] = "extractor"
            m[1:-1:2, 1] = m[1:-1:2, -2] = m[1, 2:-2:2] = m[-2, 2:-2:2] = "chest"
            m[2:-2, 2:-2] = random_map(size - 4, size - 4, {}, {"red": per_team, "blue": per_team}, seed0 + s, border_width=0)
            maps.append(m)
    else:
        maps = [random_map(size, size, dict(objs), {"red": per_team, "blue": per_team}, seed0 + s) for s in range(E)]
    return prog, np.stack([prog.class_map(m) for m in maps])


CROWDED = [(8, 11, {"wall": 3, "extractor": 4, "chest": 2}), (12, 13, {"wall": 3, "extractor": 4, "chest": 2}), (3, 9, "ring")]


@pytest.mark.parametrize("per_team,size,objs", CROWDED)
def test_crowded_arenas_three_ways(per_team, size, objs, monkeypatch):
    """Runs end early and often — a neighbour with on_use ahead, a cell vacated or entered earlier in the tick, a swap — so
    prefetched records are dropped and loaded again at the next trip.  16 envs x 40 steps."""
    prog, cms = _crowded(per_team, size, objs, 16, 900 + 10 * per_team + size)
    (ran, stale), _ = _run_trio(prog, cms, _mixed_actions(prog, 16, 40, 7 + per_team + size), monkeypatch)
    assert ran > 0 and stale > 0, (ran, stale)


@pytest.mark.parametrize("per_team,size,objs", CROWDED)
def test_crowded_arenas_against_the_oracle(per_team, size, objs, monkeypatch):
    """The same arenas and traces, default engine against the oracle after every step, 16 envs x 40 steps."""
    import torch
    for k in (SERIAL, NO_MF):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(COUNT, "1")
    E = 16
    prog, cms = _crowded(per_team, size, objs, E, 900 + 10 * per_team + size)
    A, seeds = prog.num_agents, np.arange(E, dtype=np.uint32) + 5
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    assert eng.move_fast in (1, 3) and eng.act_variant == 0
    oracles = [op.OracleSim(prog, cms[i], int(seeds[i])) for i in range(E)]
    for o in oracles:
        o.reinit_buffers()
    for t, (a, v) in enumerate(_mixed_actions(prog, E, 40, 7 + per_team + size)):
        eng.actions.copy_(torch.from_numpy(a)); eng.vibe_actions.copy_(torch.from_numpy(v)); torch.cuda.synchronize()
        eng.step()
        snap = eng.snapshot()
        for i, o in enumerate(oracles):
            o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
            hp.compare_snapshots(o.snapshot(), {k: x[i * A:(i + 1) * A] for k, x in snap.items()}, f"env {i} step {t + 1}")
    bits = 0
    for o in oracles:
        bits |= int(o.error)
    assert eng.poll_errors()[0] == bits
    for i, o in enumerate(oracles):
        for x, y in zip(o.raw_stats(), eng.raw_stats(i)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), f"stats of env {i} differ from the oracle's"
    ran, stale = eng.move_fast_counts()
    eng.close()
    assert ran > 0 and stale > 0, (ran, stale)


def test_swap_displaces_an_agent_after_its_own_turn(monkeypatch):
    """The preset's agent on_use swaps same-team neighbours.  Two rows of eight team mates side by side; every agent either
    stays (a noop: consumed by the run-ahead) or steps west or east into its neighbour (a swap: the general path).  In the 64
    envs' shuffled orders an agent that stays is displaced before its turn in some (stale entry: moved, prev_location and
    steps_without_motion of the general path) and after it in others — then `moved` and prev_location are those of its own
    turn: the epilogue must not look at the position the swap left.  Both are in the digest and the next step's bookkeeping."""
    prog = _rung3()
    rows = ["#" * 32] + ["#" + "." * 30 + "#" for _ in range(30)] + ["#" * 32]
    rows[5] = "#..." + "r" * 8 + "." * 19 + "#"
    rows[9] = "#..." + "b" * 8 + "." * 19 + "#"
    cm = prog.class_map(ascii_map(rows, {"#": "wall", ".": "empty", "r": "agent.red", "b": "agent.blue"}))
    E, A, steps = 64, prog.num_agents, 30
    cms = np.stack([cm] * E)
    names = list(prog.action_names)
    ids = np.array([names.index("noop"), names.index("move_west"), names.index("move_east")], dtype=np.int32)
    rng = np.random.default_rng(77)
    actions = [(ids[rng.choice(3, E * A, p=[0.5, 0.25, 0.25])], np.zeros(E * A, np.int32)) for _ in range(steps)]
    (ran, stale), err = _run_trio(prog, cms, actions, monkeypatch, preset=True)
    assert err == 0 and ran > E * A * steps // 4 and stale > E, (ran, stale)   # (displaced before the own turn: stale)


def test_invalid_wrong_stream_and_noop_envs(monkeypatch):
    """Per-env action patterns on the preset's shape, 70 envs x 24 steps: env 0 all ids invalid in both streams (every position
    of the order, the first and the last included, ends a run); env 1 every primary id a wrong-stream (vibe) id: the run
    consumes all 16 without a store; env 2 all noops; env 3 valid primaries under an all-invalid vibe stream; env 4 a noop
    everywhere but ONE invalid id that walks through the agents (wherever the shuffle puts it: 24 positions drawn); the
    others mixed with one invalid id each."""
    prog = _rung3()
    E, A, n_act, steps = 70, prog.num_agents, len(prog.action_names), 24
    names = list(prog.action_names)
    noop = names.index("noop")
    vibes = np.array([i for i, nm in enumerate(names) if nm.startswith("change_vibe")], dtype=np.int32)
    assert len(vibes) > 0
    rng = np.random.default_rng(3)
    actions = []
    for t, (a, v) in enumerate(_mixed_actions(prog, E, steps, 41)):
        a, v = a.reshape(E, A), v.reshape(E, A)
        a[0] = rng.choice([-1, -7, n_act, n_act + 3, 1 << 20], A); v[0] = rng.choice([-2, n_act + 1], A)
        a[1] = vibes[rng.integers(0, len(vibes), A)]
        a[2] = noop
        v[3] = n_act + 2
        a[4] = noop; a[4, t % A] = n_act
        for e in range(5, E):
            a[e, rng.integers(0, A)] = -1 if e & 1 else n_act
        actions.append((a.reshape(-1).astype(np.int32), v.reshape(-1).astype(np.int32)))
    (ran, stale), err = _run_trio(prog, _rung3_maps(prog, E), actions, monkeypatch, preset=True)
    assert err == 0 and ran > 3 * A * steps, (ran, stale)


def test_hashed_dirty_mask_40x40(monkeypatch):
    """1 600 cells: the dirty set is a 128-bit hashed mask (generic instance, run-time shape accessors)."""
    prog = _rung3(40, 256)
    E = 70
    cms = random_class_maps(prog, 40, 40, {"wall": 60, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    (ran, stale), err = _run_trio(prog, cms, _mixed_actions(prog, E, 40, 23), monkeypatch)
    assert err == 0 and ran > 0 and stale > 0, (ran, stale)


def test_fifteen_agents_generic_instance(monkeypatch):
    """A = 15 (7 + 8) and one action fewer (seven move directions): no preset shape — the generic instance (run-time shape, the action table read
    from the program), an odd flat run (32 x 15 elements), the helper split 8 | 7."""
    base = presets.rung3_spec()
    spec = dataclasses.replace(base, agents=list(base.agents[:7]) + list(base.agents[8:]), move_directions=list(base.move_directions[:7]))
    prog = compile_spec(spec, 32, 32, max_objects=192)
    assert prog.num_agents == 15 and len(prog.action_names) == 12
    E = 45
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 7, "blue": 8}, range(E))
    (ran, stale), err = _run_trio(prog, cms, _mixed_actions(prog, E, 60, 15), monkeypatch)
    assert err == 0 and ran > E * 15 * 60 // 4, (ran, stale)


def test_second_lean_engine_in_front(monkeypatch):
    """A lean engine created first takes constant slot 0: the trio runs on the unit compiled for the other slot."""
    prog = _rung3()
    E = 45
    cms = _rung3_maps(prog, E)
    front = BatchedMettaGrid(prog, cms[:2], np.arange(2, dtype=np.uint32), buffers="device", specialize=False)
    front.step()
    (ran, stale), err = _run_trio(prog, cms, _mixed_actions(prog, E, 40, 9), monkeypatch, preset=True)
    front.step()
    assert front.poll_errors()[0] == 0
    front.close()
    assert err == 0 and ran > 0, (ran, stale)
