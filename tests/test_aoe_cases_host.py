"""The cases of tests/aoe_cases.py, without a GPU.

1. Witnesses: every case is run on the oracle alone, with the maps, seeds and actions tests/test_gpu_aoe_local.py gives the
   envs it compares (helpers.ParityRun: env i has map seed i), and must reach what it is for — a gain that can only come
   from a source in the second bitmap word or the second chunk, an exit, every operation of `aoe_ops` once, a stat the kernel
   does not stage.  These are conditions on the inputs: a case that misses one gets another map or more steps.
2. The oracle against the REAL reference for these cases: tests/golden/vs_reference/aoe_traces.npz, written by
   tests/golden/make_aoe_vs_reference.py (digests of every caller-visible buffer per step, the final signature payload).
"""
import functools
import json
import os

import numpy as np
import pytest

import aoe_cases as ac
import helpers as hp
import oracle_py as op
from mettagrid_amd import signature as sg

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_ENVS = (0, 31, 32, 63, 64, 69)                   # tests/test_gpu_aoe_local.py
SEEDS = sorted(set(range(3)) | set(CHECK_ENVS))
E_GPU = 70
CASES = list(ac.AOE_SCENARIOS)


@functools.lru_cache(maxsize=None)
def program(name: str):
    spec_f, map_f, _, _ = hp.scenario(name)
    return hp.compile_scenario(name, spec_f(), *map_f(0).shape)


class Trace:
    """One env of a case on the oracle: per step (index 0: before the first) every agent's row, column, vibe and inventory,
    and the agent stats with their key bits."""

    def __init__(self, name: str, seed: int):
        _, map_f, self.steps, invalid = hp.scenario(name)
        self.prog = prog = program(name)
        self.cells = map_f(seed)
        o = op.OracleSim(prog, prog.class_map(self.cells), seed * 7 + 3)   # (ParityRun's env seed)
        o.reinit_buffers()
        acts, vibes = hp.make_actions(prog, seed, self.steps, invalid)
        self.agents, self._vibes, self._items, self.values, self.keys = [], [], [], [], []
        self._keep(o)
        self.fullest = 0
        for t in range(self.steps):
            o.step(acts[t], vibes[t])
            self._keep(o)
            self.fullest = max(self.fullest, int((o.snapshot()["obs"][:, :, 0] != 0xFF).sum(axis=1).max()))
        self.error = int(o.error)


    def _keep(self, o) -> None:
        raw = o.raw_objects()   # (mgx.h mgx_get_objects: id, class, r, c, vibe, alive, agent id, order length, order[13], amounts[13], ...)
        ag = raw[raw[:, 6] >= 0]
        ag = ag[np.argsort(ag[:, 6])]
        self.agents.append([(int(r), int(c)) for r, c in ag[:, 2:4]])
        self._vibes.append(ag[:, 4].copy())
        self._items.append(ag[:, 8 + 13:8 + 26].copy())
        _, _, av, at = o.raw_stats()
        self.values.append(av.copy())
        self.keys.append(at.copy())

    def stat(self, name: str, t: int = -1) -> np.ndarray:
        return self.values[t][:, self.prog.agent_stat_names.index(name)]

    def stats(self, name: str) -> np.ndarray:
        """[steps + 1, agents] values of one agent stat."""
        return np.array(self.values)[:, :, self.prog.agent_stat_names.index(name)]

    def key(self, name: str, t: int = -1) -> np.ndarray:
        return self.keys[t][:, self.prog.agent_stat_names.index(name)] != 0

    def item(self, name: str) -> np.ndarray:
        """[steps + 1, agents] amounts of one resource."""
        return np.array(self._items)[:, :, self.prog.resource_names.index(name)]

    def vibes(self) -> np.ndarray:
        return np.array(self._vibes)


@functools.lru_cache(maxsize=None)
def trace(name: str, seed: int) -> Trace:
    return Trace(name, seed)


RADIUS = {"healer": 3, "fire": 2}


def wall_row(cells: np.ndarray) -> int:
    """The first full wall row below the border: agents start below it and cannot cross it."""
    return next(r for r in range(1, cells.shape[0] - 1) if (cells[r] == "wall").all())


def out_of_reach(cells: np.ndarray, src: tuple) -> bool:
    """No cell below the wall row is within the source's radius (the nearest one is straight below it)."""
    r, _, name = src
    return wall_row(cells) + 1 - r > RADIUS[name]


def covered(src: tuple, r: int, c: int) -> bool:
    return (src[0] - r) ** 2 + (src[1] - c) ** 2 <= RADIUS[src[2]] ** 2


# ---- 1. witnesses -------------------------------------------------------------------------------------------------------------
def test_every_case_runs_clean_in_every_env_of_the_gpu_run():
    """run_parity requires that no env raises an error bit; a row one token over the budget would (the reference throws)."""
    for name in CASES:
        _, map_f, steps, _ = hp.scenario(name)
        assert steps <= 40 and max(map_f(0).shape) <= 24, name
        for seed in range(E_GPU):
            tr = trace(name, seed) if seed in SEEDS else Trace(name, seed)
            assert tr.error == 0, (name, seed, tr.error)
            assert tr.fullest < tr.prog.num_tokens, (name, seed, tr.fullest)


def test_source_counts():
    """Every count of the seed pattern stands among the envs the GPU test compares, and among the witnesses' seeds 0..2."""
    for seeds in (range(3), CHECK_ENVS):
        assert {len(ac.fixed_sources(ac.words_map(s))) for s in seeds} == {31, 32, 33}
    assert [len(ac.fixed_sources(ac.chunks_map(s))) for s in range(3)] == [88, 89, 90]
    assert [len(ac.fixed_sources(ac.chunks_map(s))) for s in CHECK_ENVS] == [88, 89, 90, 63, 64, 63]
    assert {len(ac.fixed_sources(ac.chunks_map(s))) for s in range(E_GPU)} == {63, 64, 65, 88, 89, 90}
    for s in range(3):   # the agent loop's second trip against the second chunk
        cells = ac.wide_map(s)
        assert len(ac.fixed_sources(cells)) >= 70 + s and program("aoe_chunks_wide").num_agents == 70
    kinds = [len(ac.fixed_sources(ac.wide_map(s))) for s in range(3)]
    assert kinds == [72, 73, 74]


@pytest.mark.parametrize("seed", SEEDS)
def test_aoe_words_gains_from_the_second_word(seed):
    """Shield comes from healers alone (presence delta).  Sources 0..28 stand out of reach, the reachable ones are fires
    except source 32 where there are 33: shield is gained exactly in those envs, through bit 0 of word 1."""
    tr = trace("aoe_words", seed)
    src = ac.fixed_sources(tr.cells)
    assert all(out_of_reach(tr.cells, s) for s in src[:ac.WORDS_WALLED])
    reach = [k for k, s in enumerate(src) if s[2] == "healer" and not out_of_reach(tr.cells, s)]
    assert reach == ([32] if len(src) == 33 else [])
    assert bool(tr.stat("shield.gained").sum() > 0) == (len(src) == 33)
    assert tr.stat("hp.lost").sum() > 0   # (the fires at 29..31: the high bits of word 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_aoe_chunks_gains_and_exits_from_the_second_chunk(seed):
    tr = trace("aoe_chunks", seed)
    src = ac.fixed_sources(tr.cells)
    assert all(out_of_reach(tr.cells, s) for s in src[:ac.CHUNKS_WALLED])
    reach = [k for k, s in enumerate(src) if s[2] == "healer" and not out_of_reach(tr.cells, s)]
    assert tr.stat("shield.gained").sum() > 0
    if len(src) <= 64:
        return   # one chunk (and, at 65 of the engine's 90, sources [64, 90) that do not exist)
    assert min(reach) >= 64, "a healer of the first chunk is within reach"
    assert tr.stat("shield.lost").sum() > 0, "no agent left a healer of the second chunk"
    # the deferred net deltas span the chunks: an agent stands in a fire of chunk 0 and in a source of chunk 1 at once
    both = [(t, a) for t in range(1, tr.steps + 1) for a, (r, c) in enumerate(tr.agents[t])
            if any(covered(s, r, c) for s in src[ac.CHUNKS_WALLED:64]) and any(covered(s, r, c) for s in src[64:])]
    assert both, "no agent is covered by sources of both chunks in one step"
    # ... and ore and energy, new to the agent, arrive in one fixed_finish (first seen: ore, then energy)
    ore, energy = tr.item("ore"), tr.item("energy")
    assert ((ore[:-1] == 0) & (ore[1:] > 0) & (energy[:-1] == 0) & (energy[1:] > 0)).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_aoe_chunks_wide_reaches_agents_and_sources_past_64(seed):
    tr = trace("aoe_chunks_wide", seed)
    gained = tr.stat("shield.gained")
    assert gained[:64].sum() > 0 and gained[64:].sum() > 0          # both trips of the agent loop
    assert tr.stat("hp.lost")[64:].sum() > 0                          # (the mobile sting or an attack)


@pytest.mark.parametrize("seed", SEEDS)
def test_aoe_ops_every_operation_fires(seed):
    tr = trace("aoe_ops", seed)
    near, far, n = ac.OPS_PEN_NEAR, ac.OPS_PEN_FAR, tr.steps
    assert not [a for a in tr.prog.action_names if "vibe" in a], "vibes must change through area effects alone"
    for a in (near, far):   # penned in: they never move
        assert len({tr.agents[t][a] for t in range(n + 1)}) == 1
    probe = next(s for s in ac.fixed_sources(tr.cells) if s[2] == "probe")
    dist = [abs(tr.agents[0][a][1] - probe[1]) + abs(tr.agents[0][a][0] - probe[0]) for a in (near, far)]
    assert dist == [1, 2]
    # MaxDistanceFilter(1) inside a radius of 3: both outcomes
    assert tr.stat("near.hits")[near] == n and not tr.key("near.hits")[far]
    # PeriodicFilter: present on some steps and absent on others, the same ones for both
    pulses = [tr.stat("pulse.hits", t)[[near, far]] for t in range(n + 1)]
    assert 0 < pulses[-1][near] < n and pulses[-1][near] == pulses[-1][far]
    assert {float(b[near] - a[near]) for a, b in zip(pulses, pulses[1:])} == {0.0, 1.0}
    # ChangeVibe by an area effect, and effect_self: nobody but the penned agent itself is within its own record's radius
    vibes = tr.vibes()
    assert (vibes[1:, near] != vibes[:-1, near]).any() and (vibes[1:] != vibes[:-1]).any()
    assert tr.stat("x11.gained")[near] > 0 and tr.stat("x11.gained")[far] > 0
    # ClearInventory: x12 is named by the all-items form alone; the list form empties x8 and leaves x12
    x8, x12 = tr.item("x8"), tr.item("x12")
    assert tr.stat("x12.lost").sum() > 0
    assert x8[0, far] > 0 and x8[-1, far] == 0 and (x12[:, far] == x12[0, far]).all() and x12[0, far] > 0
    # GameValueMutation on a stat and on an inventory value (tuner: x10 += x11 + 1; on_tick: x7 += 1; on_enter: gear += 2)
    assert tr.stat("zone.ticks").sum() > 0 and tr.stat("x10.gained").sum() > 0 and tr.stat("x7.gained").sum() > 0
    # the modifier branch: nothing but limit enforcement lowers carbon to anything but 0
    carbon, gear = tr.item("carbon"), tr.item("gear")
    drop = (carbon[1:] < carbon[:-1]) & (carbon[1:] > 0)
    lost = tr.stats("gear.lost")
    assert drop.any() and (lost[1:] > lost[:-1])[drop].all()
    # erase from the order word, and re-insertion at its head (on_enter hands gear back)
    assert ((gear[:-1] > 0) & (gear[1:] == 0)).any()
    # territory handlers
    assert tr.stat("zone.entered").sum() > 0 and tr.stat("x7.lost").sum() > 0


def test_aoe_ops_reinserts_an_erased_item():
    """gear falls to 0 (erased from the order word) and comes back (inserted at its head) in at least one checked env."""
    back = 0
    for seed in SEEDS:
        gear = trace("aoe_ops", seed).item("gear")
        back += int(((gear[:-1] == 0) & (gear[1:] > 0)).any())
    assert back > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_aoe_stats_writes_stats_the_kernel_does_not_stage(seed):
    """m28..m33 are named after the 32 staged ids (aoe_cases.STATS_UNSTAGED): the key of each exists, m30 and m33 are never
    0, m28 (shield) is 0 for some agent with its key set; so are the per-resource stats of the high resources."""
    tr = trace("aoe_stats", seed)
    names = tr.prog.agent_stat_names
    named = ["near.hits", "pulse.hits", "zone.entered", "zone.ticks"] + [f"m{i:02d}" for i in range(ac.STATS_EXTRA)]
    assert len(named) - 32 == len(ac.STATS_UNSTAGED) and named[32:] == list(ac.STATS_UNSTAGED)
    assert all(names.index(x) < 256 for x in named)
    assert max(names.index(x) for x in named) >= 64, "no staged id beyond the second touched word"
    for x in ac.STATS_UNSTAGED:
        assert tr.key(x).any(), x
    for x in ("m30", "m33"):
        assert (tr.stat(x)[tr.key(x)] > 0).all() and tr.key(x).any()
    assert any((tr.key("m28", t) & (tr.stat("m28", t) == 0)).any() for t in range(tr.steps + 1))
    assert tr.stat("x12.lost").sum() > 0 and tr.stat("x10.gained").sum() > 0 and tr.key("x11.amount").any()


# ---- 2. the oracle against the real reference -------------------------------------------------------------------------------
GOLD_PATH = os.path.join(HERE, "golden", "vs_reference", "aoe_traces.npz")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("seed", [5, 6])
def test_oracle_equals_reference(name, seed):
    gold = np.load(GOLD_PATH)
    spec_f, map_f, steps, invalid = hp.scenario(name)
    cells = map_f(seed)
    prog = program(name)
    want = gold[f"{name}_s{seed}/digests"]
    assert want.shape == (steps + 1, len(hp.SNAPSHOT_KEYS))
    ora = op.OracleSim(prog, prog.class_map(cells), seed)
    acts, vibes = hp.make_actions(prog, seed, steps, invalid)

    def check(t):
        got = hp.snapshot_digests(ora.snapshot())
        bad = [k for k, a, b in zip(hp.SNAPSHOT_KEYS, got, want[t]) if a != b]
        assert not bad, f"{name} seed {seed} step {t}: {bad} differ from the reference"

    check(0)
    for t in range(steps):
        ora.step(acts[t], vibes[t])
        check(t + 1)
    pa = json.loads(bytes(gold[f"{name}_s{seed}/payload"]).decode())
    pb = json.loads(json.dumps(hp.payload_from_raw(prog, ora.raw_objects(), ora.current_stat_reward(), ora.raw_stats(),
                                                   ora.snapshot(), ora.current_step, seed)))
    assert pa == pb, hp.diff_payload(pa, pb)
