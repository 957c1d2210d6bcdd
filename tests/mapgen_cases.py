"""Shapes, recipes and seeds shared by tests/test_mapgen_device.py (CPU) and tests/test_gpu_mapgen.py (GPU)."""
import dataclasses
import functools
import os

import numpy as np

from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.mapgen import TEAM0, RandomMapSpec

HERE = os.path.dirname(os.path.abspath(__file__))
# inner areas: the no-swap and one-swap ends, and the end of the array on / before / behind a block of 64 outputs (128 halves)
AREAS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 900)
BORDERS = (0, 1, 2)
SEEDS = np.array([0, 1, 2 ** 31, 2 ** 32 - 1] + [int(s) for s in np.random.default_rng(20261017).integers(0, 2 ** 32, 20)], dtype=np.uint64)


def shape(area: int, border: int) -> tuple:
    ih, iw = (30, 30) if area == 900 else (1, area)
    return ih + 2 * border, iw + 2 * border


@functools.lru_cache(maxsize=None)
def case(area: int, border: int, two_teams: bool):
    """(prog, RandomMapSpec): rung-3 rules with as many agents as the recipe places, on a map of that inner area."""
    n_red = min(8, max(1, area // 4))
    n_blue = min(8, max(1, area // 4)) if two_teams and area >= 2 else 0
    base = presets.rung3_spec()
    red = [a for a in base.agents if a.team_id == 0][:n_red]
    blue = [a for a in base.agents if a.team_id == 1][:n_blue]
    H, W = shape(area, border)
    prog = compile_spec(dataclasses.replace(base, agents=red + blue), H, W, max_objects=192)
    objects = {k: v for k, v in {"wall": area // 4, "extractor": min(8, area // 8), "chest": min(4, area // 16)}.items() if v}
    agents = ({"red": n_red, "blue": n_blue} if n_blue else {"red": n_red}) if two_teams else n_red
    return prog, RandomMapSpec(H, W, objects, agents, border_width=border)


def maps_from_perm(low, perm) -> np.ndarray:
    """The class map of a lowered recipe whose inner array was shuffled into ``inner[perm]`` — cell by cell."""
    inner = [int(low.inner[p]) for p in perm]
    seen = [0] * low.n_teams
    for i, v in enumerate(inner):
        if v >= TEAM0:
            t = v - TEAM0
            inner[i] = int(low.rename[low.rename_off[t] + seen[t]])
            seen[t] += 1
    out = np.full((low.height, low.width), low.border_code, np.uint16)
    b = low.border_width
    out[b:b + low.ih, b:b + low.iw] = np.array(inner, np.uint16).reshape(low.ih, low.iw)
    return out


def fixture():
    """tests/golden/mapgen/random_maps.npz: numpy's own shuffles of arange(area) for a dozen (area, seed) pairs."""
    z = np.load(os.path.join(HERE, "golden", "mapgen", "random_maps.npz"))
    return [(int(a), int(s), z[f"perm_{k}"]) for k, (a, s) in enumerate(zip(z["areas"], z["seeds"]))]
