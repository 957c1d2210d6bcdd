"""Host side of rendering (mettagrid_amd/render.py): the text frame against the reference's own renderer as recorded in
tests/golden/render_frames.json (tests/golden/make_render_fixture.py), the numpy frame rule against frames written out by
hand, the default atlas.  No GPU."""
import json
import os

import numpy as np
import pytest

import ref_tree
from mettagrid_amd import from_reference as fr
from mettagrid_amd import render
from mettagrid_amd import spec as S
from mettagrid_amd.compiler import compile_spec

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "render_frames.json"), encoding="utf-8"))
_PROGS = {}


def scenario_prog(name):
    if name not in _PROGS:
        doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
        cells = np.asarray(doc["map"], dtype=object)
        _PROGS[name] = fr.compile_reference_config(ref_tree.load(doc["config"]), *cells.shape)
    return _PROGS[name]


def synthetic_prog():
    """A program that has the type names of the synthetic cases: eleven agents (ids 9 and 10), a dotted and an unknown type."""
    if "synthetic" not in _PROGS:
        spec = S.GameSpec(resource_names=["a"], agents=[S.AgentSpec() for _ in range(11)],
                          objects={"wall": S.ObjectSpec("wall", kind="wall"), "crate": S.ObjectSpec("crate"),
                                   "block.heavy": S.ObjectSpec("block.heavy"), "mystery": S.ObjectSpec("mystery")},
                          obs=S.ObsSpec(5, 5, 60))
        _PROGS["synthetic"] = compile_spec(spec, 8, 8)
    return _PROGS["synthetic"]


def dicts(rows) -> dict:
    out = {}
    for i, (name, r, c, agent) in enumerate(rows):
        out[i + 1] = {"type_name": name, "r": r, "c": c}
        if agent >= 0:
            out[i + 1]["agent_id"] = agent
    return out


@pytest.mark.parametrize("k", range(len(DOC["frames"])), ids=[f"{f['scenario']}-{f['step']}" for f in DOC["frames"]])
def test_ansi_equals_the_reference_frames(k):
    f = DOC["frames"][k]
    prog = scenario_prog(f["scenario"])
    cells = render.cells_from_objects(prog, dicts(f["objects"]), f["height"], f["width"])
    assert render.ansi(cells, render.class_type_names(prog), f["symbols"]) == f["text"]


def test_scenario_frames_cover_what_they_are_for():
    frames = DOC["frames"]
    assert sorted({f["scenario"] for f in frames}) == ["arena", "navigation", "spawn_in_event"]
    assert all(len([f for f in frames if f["scenario"] == n]) == 3 for n in ("arena", "navigation", "spawn_in_event"))
    spawn = [f for f in frames if f["scenario"] == "spawn_in_event"]
    assert {o[0] for o in spawn[0]["objects"]} != {o[0] for o in spawn[-1]["objects"]}   # objects appear at run time
    assert frames[0]["text"] != frames[2]["text"]


@pytest.mark.parametrize("k", range(len(DOC["synthetic"])), ids=[c["name"] for c in DOC["synthetic"]])
def test_ansi_equals_the_reference_on_synthetic_lists(k):
    case = DOC["synthetic"][k]
    prog = synthetic_prog()
    cells = render.cells_from_objects(prog, dicts(case["objects"]), case["height"], case["width"])
    assert render.ansi(cells, render.class_type_names(prog), case["symbols"]) == case["text"]


def test_synthetic_cases_are_the_ones_asked_for():
    by = {c["name"]: c for c in DOC["synthetic"]}
    assert by["no_object"]["text"] == render.DEFAULT_SYMBOLS["empty"]                   # 1x1 at (0, 0)
    assert by["interior_walls"]["text"].count("\n") == 2                               # cropped to the walls' rows 2..4
    assert "\U0001F4E6" in by["dotted_falls_back"]["text"] and "❓" in by["unknown_type"]["text"]
    assert "CC" in by["overrides"]["text"] and ".." in by["overrides"]["text"]
    assert render.AGENT_SQUARES[9] in by["agents_9_and_10"]["text"] and render.DEFAULT_SYMBOLS["agent"] in by["agents_9_and_10"]["text"]


def test_default_tables_equal_the_reference():
    assert render.DEFAULT_SYMBOLS == DOC["default_symbols"]
    assert render.AGENT_SQUARES == DOC["agent_squares"]


def test_cells_from_objects_words_and_refusals():
    prog = synthetic_prog()
    names = render.class_type_names(prog)
    crate = names.index("crate")
    cells = render.cells_from_objects(prog, {1: {"type_name": "crate", "r": 1, "c": 2, "vibe": 3},
                                             2: {"type_name": "agent", "r": 0, "c": 0, "agent_id": 10, "class_id": 4}}, 3, 4)
    assert cells.dtype == np.uint32 and cells.shape == (3, 4)
    assert cells[1, 2] == (crate + 1) | 0xFF << 16 | 3 << 24 and cells[0, 0] == 5 | 10 << 16
    assert np.count_nonzero(cells) == 2
    with pytest.raises(ValueError):
        render.cells_from_objects(prog, {1: {"type_name": "crate", "r": 3, "c": 0}}, 3, 4)
    with pytest.raises(ValueError):
        render.cells_from_objects(prog, {1: {"type_name": "nothing", "r": 0, "c": 0}}, 3, 4)


# ---- the frame rule on a 2x3 map, written out by hand ----
def hand_case(s):
    """cells: [empty, class 0, agent 1 of class 2 with vibe 2] / [class 1 with vibe 1, class 1 with vibe 3 (no such vibe), empty]."""
    cells = np.array([[0, 1 | 0xFF << 16, 3 | 1 << 16 | 2 << 24], [2 | 0xFF << 16 | 1 << 24, 2 | 0xFF << 16 | 3 << 24, 0]], np.uint32)
    tiles = np.arange(5 * s * s * 3, dtype=np.int64).reshape(5, s, s, 3) % 251
    class_tile, agent_tile = [1, 2, 3], [4, 3]      # the agent is drawn with agent_tile[1] = 3, not with its class' tile
    vibe_rgb = np.array([[9, 9, 9], [250, 0, 1], [2, 251, 3]], np.uint8)
    return cells, tiles.astype(np.uint8), class_tile, agent_tile, vibe_rgb


def test_rgb_host_scale_1_by_hand():
    cells, tiles, ct, at, vibe = hand_case(1)
    px = lambda t: tiles[t, 0, 0].tolist()  # noqa: E731
    want = np.array([[px(0), px(1), px(3)], [px(2), px(2), px(0)]], np.uint8)
    for v in (None, vibe):     # s < 3: no marker either way
        got = render.rgb_host(cells, tiles, ct, at, v)
        assert got.dtype == np.uint8 and got.shape == (2, 3, 3) and np.array_equal(got, want)


def test_rgb_host_scale_3_by_hand():
    cells, tiles, ct, at, vibe = hand_case(3)
    which = [[0, 1, 3], [2, 2, 0]]
    want = np.zeros((6, 9, 3), np.uint8)
    for r in range(2):
        for c in range(3):
            for y in range(3):
                for x in range(3):
                    want[3 * r + y, 3 * c + x] = tiles[which[r][c], y, x]
    off = render.rgb_host(cells, tiles, ct, at, None)
    assert off.shape == (6, 9, 3) and np.array_equal(off, want)
    want[0, 8] = vibe[2]       # q = 1: the top right pixel of cell (0, 2), vibe 2
    want[3, 2] = vibe[1]       # ... and of cell (1, 0), vibe 1; vibe 3 is outside the table: no marker
    on = render.rgb_host(cells, tiles, ct, at, vibe)
    assert np.array_equal(on, want) and not np.array_equal(on, off)
    both = render.rgb_host(np.stack([cells, cells[::-1].copy()]), tiles, ct, at, vibe)
    assert both.shape == (2, 6, 9, 3) and np.array_equal(both[0], on)
    assert np.array_equal(both[1], render.rgb_host(cells[::-1].copy(), tiles, ct, at, vibe))


def test_rgb_host_marker_is_the_top_right_corner():
    cells, tiles, ct, at, vibe = hand_case(8)
    on, off = render.rgb_host(cells, tiles, ct, at, vibe), render.rgb_host(cells, tiles, ct, at, None)
    changed = np.argwhere((on != off).any(axis=2))
    assert {(int(y), int(x)) for y, x in changed} <= ({(y, 16 + x) for y in range(2) for x in range(6, 8)}
                                                      | {(8 + y, x) for y in range(2) for x in range(6, 8)})
    assert np.array_equal(on[0:2, 22:24], np.broadcast_to(vibe[2], (2, 2, 3)))


@pytest.mark.parametrize("scale", [1, 2, 3, 8, 32])
def test_default_tiles(scale):
    prog = synthetic_prog()
    a, b = render.default_tiles(prog, scale), render.default_tiles(prog, scale)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    tiles, class_tile, agent_tile, vibe_rgb = a
    n_classes = len(render.class_type_names(prog))
    assert tiles.dtype == np.uint8 and tiles.shape[1:] == (scale, scale, 3)
    assert class_tile.dtype == agent_tile.dtype == np.uint16 and class_tile.shape == (n_classes,) and agent_tile.shape == (11,)
    assert vibe_rgb.dtype == np.uint8 and vibe_rgb.shape == (max(1, len(prog.vibe_names)), 3)
    assert class_tile.max() < len(tiles) and agent_tile.max() < len(tiles) and class_tile.min() > 0 and agent_tile.min() > 0
    names = render.class_type_names(prog)
    per_type = {}
    for c, n in enumerate(names):
        per_type.setdefault(n, set()).add(int(class_tile[c]))
    object_types = [n for n in per_type if n != "agent"]
    shown = [tiles[next(iter(per_type[n]))].tobytes() for n in object_types]
    assert all(len(v) == 1 for v in per_type.values()) and len(set(shown)) == len(shown)      # distinct types, distinct tiles
    assert tiles[0].tobytes() not in shown
    assert agent_tile[0] == agent_tile[10] and len({int(t) for t in agent_tile[:10]}) == 10    # ten colours, then cycling
    assert all(tiles[int(t)].tobytes() not in shown for t in agent_tile)                       # agents: a second shape
    with pytest.raises(ValueError):
        render.default_tiles(prog, 0)
    with pytest.raises(ValueError):
        render.default_tiles(prog, 33)
