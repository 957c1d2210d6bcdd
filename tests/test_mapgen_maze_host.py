"""CPU: the MapGen + Maze recipe on the host (mettagrid_amd/mapgen.py MazeGenSpec, spec_from_config, generated_class_maps, the
``integers`` draw of ``_Streams``) against the reference's own grids (tests/golden/mapgen/maze_maps.npz, written by
make_maze_maps.py) and against numpy."""
import copy

import numpy as np
import pytest

import mapgen_cases as mc
import mapgen_scene_cases as sc
import maze_cases as zc
from mettagrid_amd import early_reset as er
from mettagrid_amd import mapgen
from mettagrid_amd.mapgen import (LoweredMaze, MapGenSpec, MazeGenSpec, UnsupportedMapBuilder, generated_class_maps, maze_geometry,
                                  spec_from_config)


def test_the_table_holds_every_value_the_issue_lists():
    by_alg = {a: {(c["height"], c["width"], c["room_size"], c["wall_size"]) for c in zc.CASES if c["algorithm"] == a}
              for a in ("kruskal", "dfs")}
    want = {(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (8, 10), (7, 9), (8, 8), (5, 13), (11, 11), (17, 17), (25, 25)}
    for shapes in by_alg.values():
        assert {s + (1, 1) for s in want} <= shapes
        assert {(11, 14, 2, 1), (10, 13, 1, 2), (13, 18, 3, 2), (5, 7, 9, 1)} <= shapes
    assert by_alg["kruskal"] == by_alg["dfs"]
    assert {c["height"] * c["width"] for c in zc.CASES} >= {63, 64, 65}
    assert zc.spec_of("r11x11_full_kruskal").n_empty == zc.spec_of("r11x11_full_dfs").n_empty == 71
    big = zc.spec_of("r17x17_kruskal")
    assert big.n_walls == 144 and maze_geometry(17, 17, 1, 1)[2:] == (9, 9)      # 80 walk decisions = 81 cells - 1
    assert maze_geometry(5, 7, 9, 1) == (5, 1, 1, 1)
    # the remainder strip: empty under kruskal, wall under dfs
    assert (zc.spec_of("r2x2_kruskal").n_empty, zc.spec_of("r2x2_dfs").n_empty) == (4, 1)
    for a in ("kruskal", "dfs"):
        fill = set()
        for c in zc.CASES:
            if c["algorithm"] == a:
                spec = zc.spec_of(c["name"])
                n_sym = len(spec.instance_symbols(0))
                fill.add("none" if n_sym == 0 else "one" if n_sym == 1 else "full" if n_sym == spec.n_empty else "few")
                assert n_sym <= spec.n_empty
        assert fill == {"none", "one", "few", "full"}
    assert {(c["n"], c["mode"]) for c in zc.CASES} >= {(n, m) for n in (1, 2, 3, 4, 5) for m in ("num_agents", "instances")}
    assert {c["border_width"] for c in zc.CASES} >= {0, 1, 6} and {c["instance_border_width"] for c in zc.CASES} >= {0, 1, 3}
    assert {c["instance_border_object"] for c in zc.CASES if c["n"] > 1 and c["instance_border_width"]} == {"wall", "empty"}
    assert {type(c["agents"]) for c in zc.CASES} == {int, dict, tuple}
    # the key rules: the root stream, (k,), (k + 1,) and the lone child of a Nop
    rules = {(s.first_on_root, s.key_offset, s.instances_count > 1) for s in map(zc.spec_of, zc.NAMES)}
    assert rules >= {(True, 0, False), (True, 1, False), (True, 1, True), (False, 0, True), (False, 0, False)}
    assert {int(s) for s in zc.SEEDS[:4]} == {0, 1, 2 ** 31, 2 ** 32 - 1} and zc.FIXTURE_SEEDS == sc.FIXTURE_SEEDS


@pytest.mark.parametrize("name", zc.NAMES)
def test_spec_from_config_builds_the_references_grid(name):
    grids, configs = zc.fixture()
    spec = spec_from_config(configs[name])
    assert isinstance(spec, MazeGenSpec) and vars(spec) == vars(zc.spec_of(name))
    assert spec.instances_count == zc.BY_NAME[name]["n"]
    seeds = [s for (n, s) in grids if n == name]
    assert sorted(seeds) == sorted(zc.FIXTURE_SEEDS)
    for seed in seeds:
        got, ref = spec.random_map(seed), grids[(name, seed)]
        assert got.shape == ref.shape == (spec.map_height, spec.map_width) and (got == ref).all(), (name, seed)


@pytest.mark.parametrize("name", zc.NAMES)
def test_generated_class_maps_equals_the_string_maps(name):
    """The vectorised restatement (own SeedSequence with two-word keys, PCG64, shuffles and integers) against numpy's generators."""
    prog, spec = zc.case(name)
    got = generated_class_maps(spec, prog, zc.SEEDS)
    assert got.dtype == np.uint16 and got.shape == (len(zc.SEEDS), spec.map_height, spec.map_width)
    for i, s in enumerate(zc.SEEDS):
        assert np.array_equal(got[i], prog.class_map(spec.random_map(int(s)))), (name, int(s))
    grids, _ = zc.fixture()
    for seed in zc.FIXTURE_SEEDS:
        assert np.array_equal(generated_class_maps(spec, prog, [seed])[0], prog.class_map(grids[(name, seed)])), (name, seed)


def _connected(empty: np.ndarray) -> bool:
    seen = np.zeros_like(empty)
    todo = [tuple(np.argwhere(empty)[0])]
    seen[todo[0]] = True
    while todo:
        y, x = todo.pop()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < empty.shape[0] and 0 <= nx < empty.shape[1] and empty[ny, nx] and not seen[ny, nx]:
                seen[ny, nx] = True
                todo.append((ny, nx))
    return bool((seen == empty).all())


@pytest.mark.parametrize("name", zc.NAMES)
def test_every_room_is_connected_and_holds_the_recipes_wall_count(name):
    """Every maze is a spanning tree of the same cells: the number of empty cells is the recipe's constant n_empty, and what is
    not wall (empty cells and what the child placed on them; placed walls counted back) is one connected region."""
    c, spec = zc.BY_NAME[name], zc.spec_of(name)
    placed_walls = c["objects"].get("wall", 0)
    for seed in (0, 7, 2 ** 32 - 1):
        grid = spec.random_map(seed)
        for k in range(spec.instances_count):
            y, x = spec.room_origin(k)
            room = grid[y:y + spec.height, x:x + spec.width]
            assert np.count_nonzero(room == "wall") == spec.height * spec.width - spec.n_empty + placed_walls, (name, seed, k)
            if not placed_walls:
                assert _connected(room != "wall"), (name, seed, k)
        # the maze alone (no child): connected whatever is placed later
        bare = MazeGenSpec(**{**zc.spec_kwargs(c), "objects": {}, "agents": 0, "num_agents": None, "instances": 1})
        y, x = bare.room_origin(0)
        room = bare.random_map(seed)[y:y + bare.height, x:x + bare.width]
        assert _connected(room == "empty") and np.count_nonzero(room == "empty") == spec.n_empty


@pytest.mark.parametrize("key", [(0,), (3,), (0, 0), (2, 0), (5, 0), (4, 7)])
def test_seedseq_pool_with_one_and_two_word_keys(key):
    with np.errstate(over="ignore"):
        got = np.stack(er.generate_state8(er.seedseq_pool(zc.SEEDS, key)), axis=1).astype(np.uint32)
    for i, s in enumerate(zc.SEEDS):
        assert np.array_equal(got[i], np.random.SeedSequence(int(s), spawn_key=key).generate_state(8, np.uint32)), (int(s), key)
    if len(key) == 2:   # ... which is the first child of the key[0]-th child
        child = np.random.SeedSequence(int(zc.SEEDS[5])).spawn(key[0] + 1)[key[0]].spawn(key[1] + 1)[key[1]]
        assert np.array_equal(got[5], child.generate_state(8, np.uint32))
    if len(key) == 1:
        with np.errstate(over="ignore"):
            word = np.stack(er.generate_state8(er.seedseq_pool(zc.SEEDS, key[0])), axis=1).astype(np.uint32)
        assert np.array_equal(word, got)


def _numpy_generators(key):
    return [np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(s), spawn_key=key))) for s in zc.SEEDS]


def test_streams_integers_equals_generator_integers():
    """Interleaved m in {1, 2, 3, 4}, a different one per row and draw; m = 1 draws nothing."""
    key = (2, 0)
    st, gens = mapgen._Streams(zc.SEEDS, key), _numpy_generators(key)
    choose = np.random.RandomState(11)
    for _ in range(300):
        m = choose.randint(1, 5, len(zc.SEEDS))
        got = st.integers(m)
        want = [int(g.integers(0, int(mm))) if mm > 1 else 0 for g, mm in zip(gens, m)]
        assert got.tolist() == want
    assert st.integers(3).tolist() == [int(g.integers(0, 3)) for g in gens]   # one bound for all rows


def test_streams_integers_then_a_shuffle_on_the_same_stream():
    """An odd number of halves consumed by integers: the shuffle starts on the buffered high half, as numpy's does."""
    key = (1,)
    st, gens = mapgen._Streams(zc.SEEDS, key), _numpy_generators(key)
    for m in (4, 2, 3):
        assert st.integers(m).tolist() == [int(g.integers(0, m)) for g in gens]
    rows = np.tile(np.arange(70, dtype=np.int64), (len(zc.SEEDS), 1))
    st.shuffle(rows)
    for i, g in enumerate(gens):
        x = np.arange(70, dtype=np.int64)
        g.shuffle(x)
        assert np.array_equal(rows[i], x)
    assert st.integers(4).tolist() == [int(g.integers(0, 4)) for g in gens]


def test_the_lemire_redraw_with_a_hand_made_stream():
    """For m <= 4 only m == 3 with a half of 0 is redrawn (threshold (2**32 - 3) % 3 = 1 > low word 0); no seed the tests use
    reaches it, so the halves are hand-made: 0 is rejected, the next half decides."""
    st = mapgen._Streams(zc.SEEDS[:2])
    fed = []

    def halves(rows):
        fed.append(list(rows))
        n = len(fed)
        return np.array([0 if n == 1 else 0x80000000 if n == 2 else 0xFFFFFFFF] * len(rows), dtype=np.uint64)
    assert st.integers(3, halves=halves).tolist() == [1, 1] and len(fed) == 2        # 0 redrawn; 0x80000000 * 3 >> 32 = 1
    fed.clear()
    assert st.integers(np.array([2, 4]), halves=halves).tolist() == [0, 0] and len(fed) == 1   # a half of 0 is kept for m = 2 and 4
    fed.clear()
    assert st.integers(np.array([3, 1]), halves=halves).tolist() == [1, 0] and fed == [[0], [0]]   # only row 0 draws and redraws
    assert [(0xFFFFFFFF - (m - 1)) % m for m in (2, 3, 4)] == [0, 1, 0]   # the thresholds: only m = 3 can reject


def _config(name="r25x25_kruskal"):
    return copy.deepcopy(zc.fixture()[1][name])


def _child(d):
    return d["instance"]["children"][0]


@pytest.mark.parametrize("field,change", [
    ("instance.type", lambda d: d["instance"].update(children=[])),
    ("instance.children", lambda d: d["instance"].update(children=[])),
    ("instance.children", lambda d: d["instance"]["children"].append(copy.deepcopy(_child(d)))),
    ("instance.children[0].scene.type", lambda d: _child(d)["scene"].update(type="mettagrid.mapgen.scenes.inline_ascii.InlineAscii.Config")),
    ("instance.children[0].where", lambda d: _child(d).update(where={"tags": ["top-left"]})),
    ("instance.children[0].where", lambda d: _child(d).update(where=None)),
    ("instance.children[0].limit", lambda d: _child(d).update(limit=1)),
    ("instance.children[0].offset", lambda d: _child(d).update(offset=1)),
    ("instance.children[0].lock", lambda d: _child(d).update(lock="a")),
    ("instance.children[0].instance_id", lambda d: _child(d).update(instance_id=2)),
    ("instance.children[0].use_instance_id_for_team_assignment", lambda d: _child(d).update(use_instance_id_for_team_assignment=True)),
    ("instance.children[0].scene.children", lambda d: _child(d)["scene"].update(children=[copy.deepcopy(_child(d))])),
    ("instance.children[0].scene.transform", lambda d: _child(d)["scene"].update(transform="flip_h")),
    ("instance.children[0].scene.seed", lambda d: _child(d)["scene"].update(seed=5)),
    ("instance.room_size", lambda d: d["instance"].update(room_size={"low": 1, "high": 3})),
    ("instance.wall_size", lambda d: d["instance"].update(wall_size={"low": 1, "high": 2})),
    ("instance.algorithm", lambda d: d["instance"].update(algorithm="prim")),
    ("instance.transform", lambda d: d["instance"].update(transform="rot_90")),
    ("instance.seed", lambda d: d["instance"].update(seed=3)),
    ("instance_border_clear_radius", lambda d: d.update(instance_border_clear_radius=1)),
    ("instance_object_remap", lambda d: d.update(instance_object_remap={"hub": "hub_{instance_id}"})),
    ("instance_names", lambda d: d.update(instance_names=["a", "b", "c", "d"])),
    ("instance", lambda d: d.update(instance={"type": "mettagrid.map_builder.maze.MazeKruskalMapBuilder.Config", "width": 9, "height": 9})),
])
def test_spec_from_config_refuses_naming_the_field(field, change):
    d = _config()
    assert isinstance(spec_from_config(d), MazeGenSpec)
    change(d)
    with pytest.raises(UnsupportedMapBuilder, match="'" + field.replace("[", r"\[").replace("]", r"\]") + "'"):
        spec_from_config(d)


def test_spec_from_config_takes_sizes_as_dumped_or_plain():
    d = _config("r13x18_rs3_ws2_dfs")
    assert d["instance"]["room_size"] == {"value": 3} and d["instance"]["wall_size"] == {"value": 2}
    d["instance"].update(room_size=3, wall_size=2)
    spec = spec_from_config(d)
    assert (spec.algorithm, spec.room_size, spec.wall_size) == ("dfs", 3, 2) and vars(spec) == vars(zc.spec_of("r13x18_rs3_ws2_dfs"))


def test_spec_and_lower_refuse_what_they_must():
    prog, spec = zc.case("r25x25_kruskal")
    low = spec.lower(prog)
    assert isinstance(low, LoweredMaze) and (low.n_inst, low.rows, low.cols, low.first_on_root, low.key_offset) == (4, 2, 2, True, 1)
    assert low.symbols.shape == (4, 14) and low.n_empty == 337 and low.algorithm == 0 and low.wall_code == prog.cell_to_class["wall"] + 1
    assert [low.maze_key(k) for k in range(4)] == [None, (2,), (3,), (4,)]
    keyed = zc.spec_of("r17x17_dfs")
    assert [keyed.maze_key(k) for k in range(4)] == [(0,), (1,), (2,), (3,)]
    assert zc.spec_of("r7x9_dfs").maze_key(0) == (0,) and zc.spec_of("r8x8_dfs").maze_key(0) is None
    assert zc.spec_of("r5x13_full_dfs").maze_key(0) is None    # a lone root scene; border 0 is built as the reference builds it
    kw = zc.spec_kwargs(zc.BY_NAME["r25x25_kruskal"])
    with pytest.raises(ValueError, match="program's map is 62 x 62"):
        MazeGenSpec(**{**kw, "border_width": 5}).lower(prog)
    with pytest.raises(ValueError, match="not divisible"):
        MazeGenSpec(**{**kw, "num_agents": 15}).lower(prog)
    with pytest.raises(ValueError, match="instances asks for 3"):
        MazeGenSpec(**{**kw, "instances": 3}).lower(prog)
    with pytest.raises(ValueError, match="do not fit the 337 empty cells"):
        MazeGenSpec(**{**kw, "objects": {"wall": 334}}).lower(prog)
    with pytest.raises(ValueError, match="do not fit the 337 empty cells"):
        MazeGenSpec(**{**kw, "objects": {"wall": 334}}).random_map(0)
    MazeGenSpec(**{**kw, "objects": {"wall": 333}}).lower(prog)
    with pytest.raises(ValueError, match="more 'agent.agent' cells than agents"):
        MazeGenSpec(**{**kw, "agents": 5, "num_agents": 20}).lower(prog)
    with pytest.raises(ValueError, match="algorithm 'prim'"):
        MazeGenSpec(**{**kw, "algorithm": "prim"})
    with pytest.raises(ValueError, match="room_size and wall_size are ints"):
        MazeGenSpec(**{**kw, "room_size": 1.5})

    class Far:   # a program whose class ids reach the team codes
        words = prog.words
        agent_rename = prog.agent_rename
        cell_to_class = {**prog.cell_to_class, "wall": mapgen.TEAM0}
    with pytest.raises(ValueError, match="class ids reach the team codes"):
        spec.lower(Far)


def test_random_and_scene_recipe_results_are_unchanged():
    """The two existing recipes after ``_Streams`` learnt ``integers``: numpy's own shuffles and the reference's grids."""
    for a, seed, perm in mc.fixture():
        assert np.array_equal(mapgen.shuffled_rows(np.arange(a, dtype=np.uint16), [seed])[0], perm), (a, seed)
    prog, spec = mc.case(129, 1, True)
    assert np.array_equal(generated_class_maps(spec, prog, mc.SEEDS[:6]),
                          np.stack([prog.class_map(spec.random_map(int(s))) for s in mc.SEEDS[:6]]))
    grids, configs = sc.fixture()
    for name in ("n5_root", "n4_keyed", "a129_few", "arena_4x4"):
        prog, spec = sc.case(name)
        assert type(spec_from_config(configs[name])) is MapGenSpec
        for seed in sc.FIXTURE_SEEDS:
            assert np.array_equal(generated_class_maps(spec, prog, [seed])[0], prog.class_map(grids[(name, seed)])), (name, seed)
