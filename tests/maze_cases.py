"""Recipes, programs and seeds shared by tests/test_mapgen_maze_host.py (CPU), tests/test_gpu_mapgen_maze.py (GPU) and
tests/golden/mapgen/make_maze_maps.py (the reference's own grids): MapGen with a Maze instance scene and a Random child over the
whole room, at the smallest shapes at which the generator can still go wrong.  Every room shape is built by both algorithms.

A round of the device generator is 128 halves and the empty cells are compacted in chunks of 64 cells: the rooms of area 63 /
64 / 65 sit on the chunk boundary, 11 x 11 has 71 empty cells, 17 x 17 has 144 walls to shuffle and 80 walk decisions."""
import dataclasses
import functools
import json
import os

import numpy as np

import mapgen_scene_cases as sc
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.mapgen import MAZE_ALGORITHMS, MazeGenSpec

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS, FIXTURE_SEEDS, TEAMS = sc.SEEDS, sc.FIXTURE_SEEDS, sc.TEAMS


def _m(name, h, w, rs, ws, objects, agents, n, mode, bw, ibw, ibo="wall"):
    return dict(name=name, height=h, width=w, room_size=rs, wall_size=ws, objects=objects, agents=agents, n=n, mode=mode,
                border_width=bw, instance_border_width=ibw, instance_border_object=ibo)


# height x width of a room.  Symbols: none / one / a few / exactly the maze's empty cells ("full": the same count for both
# algorithms where the room has no remainder strip).  mode as in mapgen_scene_cases.
SHAPES = [
    _m("r1x1_full", 1, 1, 1, 1, {}, 1, 1, "num_agents", 1, 0),                           # one cell, no wall, no maze draw
    _m("r1x9", 1, 9, 1, 1, {"chest": 1}, {"red": 1, "blue": 1}, 2, "instances", 0, 1, "empty"),   # one row of cells
    _m("r9x1_none", 9, 1, 1, 1, {}, 0, 1, "instances", 1, 0),                            # one column; a lone root scene
    _m("r2x2", 2, 2, 1, 1, {}, 1, 3, "num_agents", 6, 3),                                # remainder: empty (kruskal) / wall (dfs)
    _m("r3x3", 3, 3, 1, 1, {"wall": 1, "extractor": 1}, (TEAMS, 2), 3, "instances", 1, 0),   # four walls
    _m("r8x10", 8, 10, 1, 1, {"wall": 3, "chest": 1}, 2, 2, "num_agents", 1, 1),         # remainders on both axes
    _m("r7x9", 7, 9, 1, 1, {"wall": 2}, (TEAMS, 2), 1, "instances", 1, 3),               # area 63; a lone child of a Nop
    _m("r8x8", 8, 8, 1, 1, {"extractor": 2}, (TEAMS, 2), 1, "num_agents", 1, 0),         # area 64
    _m("r5x13_full", 5, 13, 1, 1, {"wall": 30, "extractor": 7}, 4, 1, "instances", 0, 0),    # area 65; 41 empty cells; border 0
    _m("r11x11_full", 11, 11, 1, 1, {"wall": 60, "chest": 3}, {"red": 4, "blue": 4}, 1, "num_agents", 1, 0),   # 71 empty cells
    _m("r17x17", 17, 17, 1, 1, {"wall": 5, "extractor": 2}, 2, 4, "instances", 1, 1, "empty"),
    _m("r25x25", 25, 25, 1, 1, {"wall": 10}, {"red": 2, "blue": 2}, 4, "num_agents", 6, 0),  # arena size
    _m("r11x14_rs2", 11, 14, 2, 1, {"chest": 2}, 1, 5, "instances", 0, 3),
    _m("r10x13_ws2", 10, 13, 1, 2, {"wall": 2}, (TEAMS, 1), 5, "num_agents", 1, 1, "empty"),
    _m("r13x18_rs3_ws2", 13, 18, 3, 2, {}, 2, 3, "num_agents", 1, 3, "empty"),
    _m("r5x7_rs9", 5, 7, 9, 1, {}, 1, 4, "instances", 1, 1),                             # room_size clamped: one 5 x 5 cell
]
CASES = [dict(s, name=f"{s['name']}_{a}", algorithm=a) for s in SHAPES for a in MAZE_ALGORITHMS]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def spec_kwargs(c) -> dict:
    """The MazeGenSpec arguments of a case."""
    return dict(sc.spec_kwargs(c), algorithm=c["algorithm"], room_size=c["room_size"], wall_size=c["wall_size"])


def spec_of(name: str) -> MazeGenSpec:
    return MazeGenSpec(**spec_kwargs(BY_NAME[name]))


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(prog, MazeGenSpec): rung-3 rules with as many agents as the recipe places, on a map of the recipe's size."""
    spec = spec_of(name)
    return program(spec, sc._agents(BY_NAME[name])), spec


def program(spec, agents, **rules):
    base = dataclasses.replace(presets.rung3_spec(), agents=agents, **rules)
    return compile_spec(base, spec.map_height, spec.map_width, max_objects=sc.object_slots(spec))


@functools.lru_cache(maxsize=None)
def fixture():
    """{(case name, seed): the reference's grid [H][W] of strings} from tests/golden/mapgen/maze_maps.npz, and
    {case name: the config's model_dump(mode="json")} from maze_cases.json."""
    d = os.path.join(HERE, "golden", "mapgen")
    with open(os.path.join(d, "maze_cases.json")) as f:
        cases = json.load(f)
    z = np.load(os.path.join(d, "maze_maps.npz"))
    grids = {}
    for name, rec in cases.items():
        symbols = np.array(rec["symbols"])
        for seed in rec["seeds"]:
            grids[(name, seed)] = symbols[z[f"{name}_{seed}"]]
    return grids, {name: rec["config"] for name, rec in cases.items()}
