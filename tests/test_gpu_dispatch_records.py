"""GPU: the dispatch records of the fixed-shape lean world kernels (csrc/mgx_world.h MgxDispatchRecs: a general-path move holds
class, agent index, vibe, order word and inventory row of the acting agent and of the object in the cell ahead in registers,
writes through, and reads neither object from memory again until its handler chain is over).  The default engine — on the
instance compiled for the preset's shape (a run-time specialised kernel: tests/test_gpu_jit_world_records.py) — against three references that keep plain memory
accesses: a twin on the handler interpreter (MGX_NO_GEN=1: run-time-shape kernel), a twin without run-ahead
(MGX_NO_MOVE_FAST=1: every action takes the general path of the run-time-shape kernel) and the oracle on envs 0, 31, 32 and 44.
After EVERY step: state digest, observations, rewards, terminals, action_success and executed actions; after every tenth step
and the last: every stat and every object record (inventories, their iteration order, vibes).

All preset cases run the preset's own program (32x32, 8 + 8 agents, 192 slots) at 45 envs — one whole wavefront and one of 13 —
on maps that crowd the agents into a corner pen or a ring of extractors and chests, so that the general path is dense: at
least one action in four must take it, by the engine's run-ahead counters and, independently, by a count on the oracle's
state in front of every step (moves whose cell ahead holds an object with on_use)."""
import dataclasses

import numpy as np
import pytest

import helpers as hp
import jit_cases as jc
import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_class_maps, random_map

pytestmark = pytest.mark.gpu

NO_GEN, NO_MF, COUNT = "MGX_NO_GEN", "MGX_NO_MOVE_FAST", "MGX_MOVE_FAST_COUNT"
E45 = 45
DELTA = {"north": (-1, 0), "south": (1, 0), "west": (0, -1), "east": (0, 1),
         "northwest": (-1, -1), "northeast": (-1, 1), "southwest": (1, -1), "southeast": (1, 1)}


def _rung3():
    return compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)


def _engines(prog, cms, seeds, monkeypatch, preset):
    """(default, interpreter twin, twin without run-ahead).  preset: the default engine must run the preset's instance."""
    for k in (NO_GEN, NO_MF):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(COUNT, "1")
    new = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.setenv(NO_GEN, "1")
    interp = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(NO_GEN)
    monkeypatch.setenv(NO_MF, "1")
    slow = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    monkeypatch.delenv(NO_MF)
    monkeypatch.delenv(COUNT)
    assert new.world_variant == (3 if preset else 0), new.world_variant
    assert new.move_fast in (1, 3) and new.dispatch_pairs == 1 and new.act_variant == 0
    assert interp.world_variant == 0 and interp.handler_variant == 0, (interp.world_variant, interp.handler_variant)
    assert slow.world_variant == 0 and slow.move_fast == 0
    return new, interp, slow


def _same_objects_and_stats(engines, oracles, E, where):
    recs = [g.raw_objects_batch(range(E)) for g in engines]
    for other in recs[1:]:
        for i in range(E):
            assert np.array_equal(recs[0][i], other[i]), f"{where}: object records (inventories) of env {i} differ"
    for i in range(E):
        stats = [g.raw_stats(i) for g in engines]
        for other in stats[1:]:
            for x, y in zip(stats[0], other):
                assert np.array_equal(x, y), f"{where}: stats of env {i} differ"
    for i, o in oracles.items():
        assert np.array_equal(np.asarray(o.raw_objects()), recs[0][i]), f"{where}: object records of env {i} differ from the oracle's"
        for x, y in zip(o.raw_stats(), engines[0].raw_stats(i)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), f"{where}: stats of env {i} differ from the oracle's"


def _on_use_ahead(prog, o, a):
    """Moves of one env's action row whose cell ahead holds an object with on_use, on the oracle's state in front of the step."""
    recs = np.asarray(o.raw_objects())
    usable = {(int(r[2]), int(r[3])) for r in recs if r[5] and prog.class_cells[int(r[1])] != "wall"}
    at = {int(r[6]): (int(r[2]), int(r[3])) for r in recs if r[6] >= 0}
    n = 0
    for ai, act in enumerate(a):
        name = prog.action_names[act] if 0 <= act < len(prog.action_names) else ""
        if name.startswith("move_"):
            dr, dc = DELTA[name[5:]]
            n += (at[ai][0] + dr, at[ai][1] + dc) in usable
    return n


def _run(prog, cms, actions, monkeypatch, preset=True, setup=None, dense=False):
    """actions: (primary, vibe) int32 [E * A] per step.  setup(engine or oracle, env or None): inventories in front of step 1."""
    E, A = len(cms), prog.num_agents
    seeds = np.arange(E, dtype=np.uint32) * 3 + 11
    engines = _engines(prog, cms, seeds, monkeypatch, preset)
    new = engines[0]
    oracles = {i: op.OracleSim(prog, cms[i], int(seeds[i])) for i in jc.oracle_envs(E)}
    try:
        for o in oracles.values():
            o.reinit_buffers()
        if setup is not None:
            for g in engines:
                for i in range(E):
                    setup(g, i)
            for o in oracles.values():
                setup(o, None)
        ahead = 0
        for t, (a, v) in enumerate(actions):
            for i, o in oracles.items():
                ahead += _on_use_ahead(prog, o, a[i * A:(i + 1) * A])
            jc.step_engines(engines, a, v)
            for other, name in ((engines[1], "interpreter twin"), (engines[2], "twin without run-ahead")):
                jc.same_everywhere(new, other, f"default engine vs {name}, step {t + 1}")
            snap = new.snapshot()
            for i, o in oracles.items():
                o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
                hp.compare_snapshots(o.snapshot(), {k: x[i * A:(i + 1) * A] for k, x in snap.items()}, f"env {i} step {t + 1} (oracle)")
            if t % 10 == 9 or t == len(actions) - 1:
                _same_objects_and_stats(engines, oracles, E, f"step {t + 1}")
        errs = [g.poll_errors()[0] for g in engines]
        bits = 0
        for o in oracles.values():
            bits |= int(o.error)
        assert errs[0] == errs[1] == errs[2] and errs[0] | bits == errs[0], (errs, bits)
        ran, stale = new.move_fast_counts()
        general = E * A * len(actions) - ran
        share, share_oracle = general / (E * A * len(actions)), ahead / (len(oracles) * A * len(actions))
        print(f"general path: {general} of {E * A * len(actions)} actions ({share:.3f}); on_use ahead on the oracle: {share_oracle:.3f}")
        if dense:
            assert share >= 0.25, f"only {share:.3f} of the actions took the general path"
            assert share_oracle >= 0.25, f"the oracle sees an on_use object ahead of only {share_oracle:.3f} of the actions"
        return general, stale
    finally:
        for g in engines:
            g.close()


def _actions(prog, E, steps, seed, move_share=0.8, invalid=True):
    rng = np.random.default_rng(seed)
    A, n_act = prog.num_agents, len(prog.action_names)
    moves = np.array([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=np.int32)
    lo, hi = (-1, n_act + 1) if invalid else (0, n_act)
    out = []
    for _ in range(steps):
        a = rng.integers(lo, hi, E * A).astype(np.int32)
        mv = rng.random(E * A) < move_share
        a[mv] = moves[rng.integers(0, len(moves), int(mv.sum()))]
        out.append((a, rng.integers(lo, hi, E * A).astype(np.int32)))
    return out


def _pen_maps(prog, E, seed0, objs):
    """The preset's map with all 16 agents and `objs` in an 11x11 arena in its north-west corner: 9x9 cells between the map's
    border and 19 walls of its own."""
    maps = []
    for s in range(E):
        m = random_map(32, 32, {}, 0, 0)
        m[10, 1:11] = "wall"
        m[1:10, 10] = "wall"
        m[1:10, 1:10] = random_map(9, 9, dict(objs), {"red": 8, "blue": 8}, seed0 + s, border_width=0)
        maps.append(prog.class_map(m))
    return np.stack(maps)


def _ring_maps(prog, E, seed0):
    """Six agents on the 5x5 cells inside a 7x7 ring of extractors and chests (a 9x9 arena with the map's border), the other
    ten in a second, open pen of 4x6 cells below it: most moves meet an object with on_use."""
    maps = []
    for s in range(E):
        m = random_map(32, 32, {}, 0, 0)
        m[1:8, 1:8] = "extractor"
        m[1:8:2, 1] = m[1:8:2, 7] = m[1, 2:7:2] = m[7, 2:7:2] = "chest"
        m[2:7, 2:7] = random_map(5, 5, {}, {"red": 3, "blue": 3}, seed0 + s, border_width=0)
        m[13, 1:8] = "wall"
        m[9:13, 7] = "wall"
        m[8, 1:8] = "wall"
        m[9:13, 1:7] = random_map(4, 6, {"chest": 2}, {"red": 5, "blue": 5}, seed0 + 500 + s, border_width=0)
        maps.append(prog.class_map(m))
    return np.stack(maps)


def test_crowded_pen_sixteen_agents(monkeypatch):
    """16 agents, 10 extractors and 6 chests on 11x11: attacks, loot, swaps, withdrawals against the agents' ore limit
    (free_space clamps the transfer), deposits (the chest's ore goes 0 -> n: insert at the head of its order word; the agent's
    n -> 0: erase), vibes that choose the extractor's handler."""
    prog = _rung3()
    cms = _pen_maps(prog, E45, 300, {"extractor": 10, "chest": 6})
    general, stale = _run(prog, cms, _actions(prog, E45, 60, 5, move_share=0.85), monkeypatch, dense=True)
    assert stale > 0


def test_ring_of_extractors_and_chests(monkeypatch):
    """Six agents inside the ring, ten in a pen of 24 cells: extractors run dry (their ore n -> 0), chests fill."""
    prog = _rung3()
    general, stale = _run(prog, _ring_maps(prog, E45, 700), _actions(prog, E45, 80, 6), monkeypatch, dense=True)


def _set(eng_or_oracle, env, agent, inv, prog):
    ids = {prog.resource_names.index(k): v for k, v in inv.items()}
    if env is None:
        eng_or_oracle.set_inventory(agent, ids)
    else:
        eng_or_oracle.set_inventory(env, agent, ids)


def test_attacks_to_zero_hit_points_and_against_armour(monkeypatch):
    """In the pen (agent ids follow the map row by row, whatever the team): agents 0-3 and 8-11 start with 1 or 2 hit points and no armour (the first hit takes them to zero: death
    stat, the order word loses hp; the regen tick brings hp back: insert at the head), agents 4-5 and 12-13 wear armour 90
    (damage 0: no update at all), agents 6-7 and 14-15 carry 60 lasers and 7 ore (every attack of theirs lands, their victims'
    loot moves ore)."""
    prog = _rung3()

    def setup(g, env):
        for a in (0, 1, 2, 3, 8, 9, 10, 11):
            _set(g, env, a, {"hp": 1 + (a & 1), "armor": 0, "ore": 3}, prog)
        for a in (4, 5, 12, 13):
            _set(g, env, a, {"armor": 90}, prog)
        for a in (6, 7, 14, 15):
            _set(g, env, a, {"laser": 60, "ore": 7}, prog)

    cms = _pen_maps(prog, E45, 1300, {"extractor": 6, "chest": 4})
    general, stale = _run(prog, cms, _actions(prog, E45, 60, 8, move_share=0.9, invalid=False), monkeypatch, setup=setup, dense=True)


def test_swapped_and_attacked_in_the_same_tick(monkeypatch):
    """Four groups `r r b` with a second `b` under the middle agent, nothing else in reach.  The first r steps east or stays (a swap
    with its team mate), the middle one west (swap), east (attack) or stays, the two b attack whoever stands in the middle cell.
    Nobody ever steps onto an empty cell, so the layout holds for the whole run; in 45 shuffled orders an agent is swapped
    and attacked later in the same tick (the records carry no positions), is another agent's target and then acts itself (its
    record comes fresh from memory: the loot took its ore, the hit its hp), and agents of different groups — disjoint
    footprints — dispatch side by side in one trip.  Which of these orders a step took is not counted: the oracle does not
    expose the order it drew.  What is asserted is the outcome under all of them (every step, every env, against the two twins
    and the oracle) and that the paired dispatch is on."""
    prog = _rung3()
    m = random_map(32, 32, {}, 0, 0)
    for g in range(4):
        c = 2 + 5 * g
        m[5, c] = m[5, c + 1] = "agent.red"
        m[5, c + 2] = m[6, c + 1] = "agent.blue"
    cm = prog.class_map(m)
    grid = np.asarray(m)
    assert (grid == "agent.red").sum() == 8 and (grid == "agent.blue").sum() == 8
    E, A, steps = E45, prog.num_agents, 60
    cms = np.stack([cm] * E)
    names = list(prog.action_names)
    noop, west, east, north = (names.index(k) for k in ("noop", "move_west", "move_east", "move_north"))
    # agent ids follow the map row by row, whatever the team: group g holds 3 g, 3 g + 1 (red) and 3 g + 2 (blue), row 6 12 + g
    reds_first, reds_mid = [0, 3, 6, 9], [1, 4, 7, 10]
    blue_row5, blue_row6 = [2, 5, 8, 11], [12, 13, 14, 15]
    rng = np.random.default_rng(21)
    actions = []
    for _ in range(steps):
        a = np.full((E, A), noop, np.int32)
        a[:, reds_first] = rng.choice([noop, east], (E, 4), p=[0.3, 0.7])
        a[:, reds_mid] = rng.choice([noop, west, east], (E, 4), p=[0.2, 0.4, 0.4])
        a[:, blue_row5] = rng.choice([noop, west], (E, 4), p=[0.3, 0.7])
        a[:, blue_row6] = rng.choice([noop, north], (E, 4), p=[0.3, 0.7])
        actions.append((a.reshape(-1), np.zeros(E * A, np.int32)))

    def setup(g, env):
        for ag in range(A):
            _set(g, env, ag, {"laser": 40, "ore": 2 + ag % 5, "hp": 100 if ag % 3 else 2}, prog)

    general, stale = _run(prog, cms, actions, monkeypatch, setup=setup, dense=True)


def test_fifteen_agents_run_time_shape_kernel(monkeypatch):
    """A = 15 with 12 actions: no preset shape — the run-time-shape kernel, which holds no records."""
    base = presets.rung3_spec()
    spec = dataclasses.replace(base, agents=list(base.agents[:7]) + list(base.agents[8:]), move_directions=list(base.move_directions[:7]))
    prog = compile_spec(spec, 32, 32, max_objects=192)
    assert prog.num_agents == 15 and len(prog.action_names) == 12
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 7, "blue": 8}, range(E45))
    _run(prog, cms, _actions(prog, E45, 60, 15, move_share=2 / 3), monkeypatch, preset=False)
