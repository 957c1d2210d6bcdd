"""Cases of the lane-per-agent area-effect kernel (mgx_aoe_kernel: csrc/mgx_aoe.hip, csrc/mgx_aoe_local.h) beyond what
helpers.SCENARIOS reach: more than 32 and more than 64 fixed sources per env (second bitmap word, second staging chunk,
envs with fewer sources than the engine's capacity), more than 64 agents crossed with more than 64 sources, every filter
and mutation the host analysis admits (mgx_aoe_is_target_local), and more agent stats than the kernel stages in LDS.

AOE_SCENARIOS has the usual (spec factory, map factory(seed), steps, allow invalid action indices) tuples;
helpers.scenario() looks here too.  tests/test_aoe_cases_host.py shows on the oracle that every case reaches what it is
for and replays the real reference's traces; tests/test_gpu_aoe_local.py runs the kernel.  No tests here.

Registration order.  Fixed sources register in row-major order of the map's cells (mgx_init_kernel, and the oracle and
the reference with it), AoE records of one object in class order.  The maps below put the sources with the LOW indices
behind a wall row, farther from any cell an agent can reach than their radius: whatever an agent gains from the walled-off
class can then only come from a source with a high index (word 1 of the agent's bitmap, or the second chunk).
"""
from __future__ import annotations

import copy

import numpy as np

import helpers as hp
from mettagrid_amd import presets
from mettagrid_amd import spec as S

A, T = S.ACTOR, S.TARGET


# ---- maps -------------------------------------------------------------------------------------------------------------------
def layout(height: int, width: int, seed: int, top=(), gap: int = 0, fixture=(), chars=None, first=(), scatter=(), other=None,
           agents=(), anchor=None) -> np.ndarray:
    """A bordered map in four bands, top to bottom:
      * ``top``: symbols filled row-major from the first inner row, then ``gap`` empty rows and a full wall row (no agent
        gets above it);
      * ``fixture``: rows drawn by hand (``chars`` maps a character to a cell name);
      * the random band: ``first`` + ``scatter`` are sources — cells are drawn at random, sorted row-major, and handed out
        in list order, so ``first`` registers before ``scatter``; ``other`` ({name: count}) and ``agents`` (cell names)
        fall where they fall;
      * ``anchor`` = (source, agent cell): the source in the last inner row (so it registers last of all) with the agent
        beside it (in range at step 1 wherever it moves).
    """
    g = np.full((height, width), "empty", dtype="<U50")
    g[0, :] = g[-1, :] = "wall"
    g[:, 0] = g[:, -1] = "wall"
    iw = width - 2
    r = 1
    if len(top):
        for k, name in enumerate(top):
            g[1 + k // iw, 1 + k % iw] = name
        r = 1 + (len(top) + iw - 1) // iw + gap
        g[r, :] = "wall"
        r += 1
    for line in fixture:
        for j, ch in enumerate(line):
            g[r, 1 + j] = chars[ch]
        r += 1
    last = height - 2 - (1 if anchor else 0)
    cells = [(i, j) for i in range(r, last + 1) for j in range(1, width - 1)]
    rng = np.random.default_rng(seed)
    sources = list(first) + list(scatter)
    rest = [n for n, c in (other or {}).items() for _ in range(c)] + list(agents)
    assert len(sources) + len(rest) <= len(cells), "layout: the random band is too small"
    pick = rng.permutation(len(cells))
    where = sorted(cells[i] for i in pick[:len(sources)])
    for (i, j), name in zip(where, sources):
        g[i, j] = name
    for i, name in zip(pick[len(sources):len(sources) + len(rest)], rest):
        g[cells[i]] = name
    if anchor:
        j = 2 + int(rng.integers(0, iw - 3))
        g[height - 2, j], g[height - 2, j + 1] = anchor
    return g


def fixed_sources(cells: np.ndarray) -> list:
    """[(row, col, cell name)] of a map's fixed AoE sources in registration order (one entry per AoE record)."""
    out = []
    for r in range(cells.shape[0]):
        for c in range(cells.shape[1]):
            out += [(r, c, str(cells[r, c]))] * FIXED_PER_CELL.get(str(cells[r, c]), 0)
    return out


# fixed AoE records per cell name, over all the cases below (agents carry mobile records only)
FIXED_PER_CELL = {"healer": 1, "fire": 1, "probe": 3, "rust": 1, "wiper": 1, "sweeper": 1, "tuner": 1,
                  "healer_red": 1, "healer_blue": 1, "healer_green": 1, "healer_yellow": 1}
WORDS_WALLED, CHUNKS_WALLED, CHUNKS_FIRST = 29, 50, 14


def words_counts(seed: int) -> int:
    return 31 + seed % 3


def words_map(seed: int) -> np.ndarray:
    """31, 32 or 33 fixed sources: 29 healers and fires behind the wall, then fires, and — where there are 33 — one
    healer as source 32, the only healer an agent can reach: shield comes from bit 0 of word 1 or not at all."""
    n = words_counts(seed)
    rng = np.random.default_rng(7000 + seed)
    top = np.array(["healer"] * 14 + ["fire"] * 15)
    rng.shuffle(top)
    return layout(20, 20, 7100 + seed, top=list(top), gap=2, scatter=["fire"] * (n - WORDS_WALLED - 1),
                  other={"wall": 8, "hub": 2, "wire": 6, "flag_red": 1, "flag_blue": 1, "flag_green": 1},
                  agents=["agent.red"] * 3 + ["agent.blue"] * 4 + ["agent.green"] * 4,
                  anchor=("healer" if n == 33 else "fire", "agent.red"))


def words_spec() -> S.GameSpec:
    sp = hp.rung4_spec()
    sp.obs.num_tokens = 400   # (33 sources and their wall in a 9x9 window: one token over the budget is an error in the reference)
    return sp


def chunks_counts(seed: int) -> tuple:
    """(healers, fires): 63, 64 or 65 healers; 25 fires in every other triple of seeds, so totals of 63..65 and of 88..90
    stand side by side in one engine (seeds 0..2 have the fires)."""
    return 63 + seed % 3, 25 if (seed // 3) % 2 == 0 else 0


def chunks_map(seed: int) -> np.ndarray:
    """50 healers behind the wall (sources 0..49).  With fires: 14 fires next (sources 50..63, the rest of chunk 0), then
    11 fires and the other healers mixed (chunk 1), a healer last.  Every healer an agent can reach has an index of 64 or
    more, and the fires of both chunks change hp, energy and ore of whoever stands between them."""
    nh, nfire = chunks_counts(seed)
    rng = np.random.default_rng(7200 + seed)
    mixed = np.array(["fire"] * max(0, nfire - CHUNKS_FIRST) + ["healer"] * (nh - CHUNKS_WALLED - 1))
    rng.shuffle(mixed)
    return layout(24, 24, 7300 + seed, top=["healer"] * CHUNKS_WALLED, gap=2, first=["fire"] * min(nfire, CHUNKS_FIRST),
                  scatter=list(mixed), other={"wall": 10, "hub": 2, "wire": 6, "flag_red": 2, "flag_blue": 2, "flag_green": 2},
                  agents=["agent.red"] * 3 + ["agent.blue"] * 4 + ["agent.green"] * 4, anchor=("healer", "agent.red"))


def chunks_spec() -> S.GameSpec:
    """Rung 4 whose fires name three resources, the highest first: ore and energy are new to an agent that starts with hp
    alone, so the order in which the deferred net deltas are applied (first seen: ore, energy, hp) shows in the inventory's
    iteration order; the healers' hp and energy deltas land in the same per-agent sums from the other chunk."""
    sp = hp.rung4_spec()
    sp.obs.num_tokens = 400
    sp.objects["fire"].aoes = [S.AOESpec(radius=2, filters=[], mutations=[S.ResourceDelta(T, "ore", 1), S.ResourceDelta(T, "energy", 1),
                                                                        S.ResourceDelta(T, "hp", -3)])]
    for a in sp.agents:
        a.inventory.initial = {"hp": 50}
    return sp


WIDE_AGENTS = 70


def wide_spec() -> S.GameSpec:
    sp = hp.ext_agents_spec(WIDE_AGENTS)
    sp.obs.num_tokens = 400
    return sp


def wide_map(seed: int) -> np.ndarray:
    """70 agents (two trips of the kernel's agent loop) among 72..74 healers (two chunks, staged again on the second
    trip); every agent carries the mobile AoE, so 70 mobile sources in two chunks too."""
    from mettagrid_amd.mapgen import random_map
    objs = {"wall": 12, "extractor": 6, "chest": 4, "healer_red": 18 + seed % 3, "healer_blue": 18, "healer_green": 18,
            "healer_yellow": 18, "flag_red": 1, "flag_blue": 1, "flag_green": 1, "flag_yellow": 1, "hub": 1, "wire": 3}
    return random_map(24, 24, objs, hp.team_counts(WIDE_AGENTS, presets.RUNG4_TEAMS), seed)


# ---- every operation the host analysis admits ---------------------------------------------------------------------------------
OPS_RESOURCES = ["hp", "energy", "shield", "ore", "gear", "carbon", "oxygen", "x7", "x8", "x9", "x10", "x11", "x12"]
OPS_PEN_NEAR, OPS_PEN_FAR = 0, 1   # agent ids of the two penned agents: 1 and 2 cells from the probe
OPS_FIXTURE = (".#..#.............",
               "#aP#b#S...........",
               ".#..#.............")
OPS_CHARS = {".": "empty", "#": "wall", "a": "agent.red", "b": "agent.red", "P": "probe", "S": "sweeper"}


def ops_spec() -> S.GameSpec:
    """13 resources; the AoE, territory and on_tick records use between them every filter and mutation that
    mgx_aoe_is_target_local admits.  Nothing but an area effect changes a vibe (no change_vibe actions), and vibes are read
    on the target only (the host refuses a program that reads an actor's vibe while a record changes vibes).

      probe    three records of radius 3 beside two agents penned in by walls, 1 and 2 cells away: MaxDistanceFilter(1)
               passes for the near one only; PeriodicFilter(3, 1) passes for both on every third step; each counts its hits
               in a stat (GameValueMutation on a stat); every fifth step a third record sets their vibe to "b", which
               their own effect_self record (nobody else is within its radius) answers with x11 +1 and vibe "a"
      rust     gear -1: gear is the modifier of the (carbon, oxygen, x7) limit, so the group shrinks and enforcement drops
               carbon, then oxygen (inv_update<1> -> enforce_all_limits<0> -> inv_update<0>); gear 0 erases it from the
               order word, the territory's on_enter hands 2 back (insertion at the head)
      wiper    GameValueFilter over Ratio / Max / Min inside a weighted log sum; ClearInventory of everything
      sweeper  VibeFilter on the target; ClearInventory of a list (one stands 2 cells from the far pen: it fires the step
               after that agent's vibe has gone from "b" to "a")
      tuner    ResourceFilter on the target; ChangeVibe; GameValueMutation on an inventory value with a computed delta
      agents   the mobile sting of rung 4 and an effect_self record (the agent is its own target when its vibe is "b");
               a leaf on_tick with ResourceFilter and GameValueMutation
      zone     enter / exit / presence with GameValueMutation (inventory and stat), ClearInventory and SetStat
    """
    sp = hp.rung4_spec()
    sp.resource_names = list(OPS_RESOURCES)
    sp.vibe_names = ["default", "a", "b", "c"]
    sp.change_vibe_enabled = False
    sp.move_directions = ["north", "south", "west", "east"]   # (a pen of four walls holds its agent)
    sp.on_tick = None
    sp.obs.num_tokens = 400
    tick = S.Handler([S.ResourceFilter(T, "energy", 3)], [S.GameValueMutation(S.InventoryValue("x7"), S.ConstValue(1.0), T)], "tick")
    own = S.AOESpec(radius=1, is_static=False, effect_self=True, filters=[S.VibeFilter(T, "b")],
                    mutations=[S.ResourceDelta(T, "x11", 1), S.ChangeVibe(T, "a")])
    for i, a in enumerate(sp.agents):
        a.vibe = i % 3
        a.inventory.initial = {"hp": 50, "energy": 10, "gear": 3, "carbon": 4, "oxygen": 3, "x9": 1, "x12": 2, "x8": 2}
        a.inventory.limits = list(a.inventory.limits) + [S.Limit(["carbon", "oxygen", "x7"], base=1, max=40, modifiers={"gear": 2})]
        a.on_tick = copy.deepcopy(tick)
        a.aoes = list(a.aoes) + [copy.deepcopy(own)]
    count = lambda name: S.GameValueMutation(S.StatValue(name, "agent"), S.ConstValue(1.0), T)  # noqa: E731
    rich = S.SumValue([S.RatioValue(S.InventoryValue("hp"), S.MaxValue([S.InventoryValue("energy"), S.ConstValue(1.0)])),
                       S.MinValue([S.InventoryValue("ore"), S.ConstValue(5.0)])], [0.5, 2.0], log=True)
    sp.objects.update({
        "probe": S.ObjectSpec("probe", aoes=[
            S.AOESpec(radius=3, filters=[S.MaxDistanceFilter(T, 1)], mutations=[count("near.hits")]),
            S.AOESpec(radius=3, filters=[S.PeriodicFilter(3, 1)], mutations=[count("pulse.hits")]),
            S.AOESpec(radius=3, filters=[S.PeriodicFilter(5, 2)], mutations=[S.ChangeVibe(T, "b")])]),
        "rust": S.ObjectSpec("rust", aoes=[S.AOESpec(radius=2, filters=[S.ResourceFilter(T, "gear", 1)],
                                                     mutations=[S.ResourceDelta(T, "gear", -1)])]),
        "wiper": S.ObjectSpec("wiper", aoes=[S.AOESpec(radius=2, filters=[S.GameValueFilter(T, rich, S.ConstValue(0.8))],
                                                       mutations=[S.ClearInventory(T)])]),
        "sweeper": S.ObjectSpec("sweeper", aoes=[S.AOESpec(radius=2, filters=[S.VibeFilter(T, "a")],
                                                           mutations=[S.ClearInventory(T, ["x8", "x9"])])]),
        "tuner": S.ObjectSpec("tuner", aoes=[S.AOESpec(radius=2, filters=[S.ResourceFilter(T, "energy", 5)],
                                                       mutations=[S.ChangeVibe(T, "b"),
                                                                  S.GameValueMutation(S.InventoryValue("x10"),
                                                                                      S.SumValue([S.InventoryValue("x11"), S.ConstValue(1.0)]), T)])]),
    })
    same, other = S.SharedTagPrefixFilter("team:"), S.NegFilter([S.SharedTagPrefixFilter("team:")])
    sp.territories["zone"] = S.TerritorySpec(
        tag_prefix="team:",
        on_enter=[S.Handler([], [S.GameValueMutation(S.InventoryValue("gear"), S.ConstValue(2.0), T),
                                 S.SetStat("zone.entered", S.SumValue([S.StatValue("zone.entered", "agent"), S.ConstValue(1.0)]),
                                           scope="agent", entity=T)])],
        on_exit=[S.Handler([same], [S.ClearInventory(T, ["x7"]), S.ResourceDelta(T, "energy", -1)])],
        presence=[S.Handler([same], [S.ResourceDelta(T, "energy", 1), count("zone.ticks")]),
                  S.Handler([other], [S.ResourceDelta(T, "hp", -1)])])
    return sp


def ops_map(seed: int) -> np.ndarray:
    return layout(18, 20, 7400 + seed, fixture=OPS_FIXTURE, chars=OPS_CHARS,
                  scatter=["rust"] * 5 + ["wiper"] * 3 + ["sweeper"] * 2 + ["tuner"] * 3 + ["healer"] * 2,
                  other={"wall": 6, "hub": 1, "wire": 3, "flag_red": 2, "flag_blue": 2, "flag_green": 2},
                  agents=["agent.red"] * 2 + ["agent.blue"] * 4 + ["agent.green"] * 4)


# ---- more stats than the kernel stages ----------------------------------------------------------------------------------------
STATS_EXTRA = 34
# mgx_aoe_collect_stats stages at most 32 ids: first the ids SetStat / game-value mutations and value code name, in record
# order (AoE records, territory handlers, on_tick handlers), then gained / lost / amount by resource index.  The records of
# ops_spec name 4 (near.hits, pulse.hits, zone.entered, zone.ticks), the handler below 34 more: m00..m27 fill the 32 cells,
# m28..m33 and every per-resource stat of the 13 resources take the kernel's HBM path.
STATS_UNSTAGED = ("m28", "m29", "m30", "m31", "m32", "m33")


def stats_value(i: int):
    item = S.InventoryValue(OPS_RESOURCES[i % 13])
    if i % 3 == 0:
        return S.SumValue([item, S.ConstValue(1.0)])          # never 0
    if i % 3 == 1:
        return item                                            # may be 0: the key exists all the same
    return S.SumValue([S.StatValue(f"m{i:02d}", "agent"), S.ConstValue(1.0)])   # reads its own cell first


def stats_spec() -> S.GameSpec:
    sp = ops_spec()
    zone = sp.territories["zone"]
    zone.presence = list(zone.presence) + [S.Handler([], [S.SetStat(f"m{i:02d}", stats_value(i), scope="agent", entity=T)
                                                          for i in range(STATS_EXTRA)])]
    return sp


AOE_SCENARIOS = {
    # name: (spec factory, map factory(seed), steps, allow invalid action indices) as in helpers.SCENARIOS
    "aoe_words": (words_spec, words_map, 30, False),
    "aoe_chunks": (chunks_spec, chunks_map, 40, False),
    "aoe_chunks_wide": (wide_spec, wide_map, 16, False),
    "aoe_ops": (ops_spec, ops_map, 40, False),
    "aoe_stats": (stats_spec, ops_map, 24, True),
}
