"""CPU: the MapGen + Random scene recipe on the host (mettagrid_amd/mapgen.py MapGenSpec, spec_from_config, generated_class_maps)
against the reference's own grids (tests/golden/mapgen/mapgen_maps.npz, written by make_mapgen_maps.py) and against numpy."""
import copy

import numpy as np
import pytest

import mapgen_cases as mc
import mapgen_scene_cases as sc
from mettagrid_amd import early_reset as er
from mettagrid_amd import mapgen
from mettagrid_amd.mapgen import MapGenSpec, RandomMapSpec, UnsupportedMapBuilder, generated_class_maps, spec_from_config

ALL = [c["name"] for c in sc.CASES + sc.ARENA_FULL]
NAMES = [c["name"] for c in sc.CASES]


def test_the_table_holds_every_value_the_issue_lists():
    areas = {c["height"] * c["width"] for c in sc.CASES}
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 625} <= areas
    n_sym = {(sc.spec_of(n).lower(sc.case(n)[0]).n_sym, sc.BY_NAME[n]["height"] * sc.BY_NAME[n]["width"]) for n in NAMES}
    assert {0, 1, 2} <= {s for s, _ in n_sym} and any(2 < s < a for s, a in n_sym) and any(s == a > 2 for s, a in n_sym)
    assert {(c["n"], c["mode"]) for c in sc.CASES} >= {(n, m) for n in (1, 2, 3, 4, 5) for m in ("num_agents", "instances")}
    assert {c["border_width"] for c in sc.CASES} >= {0, 1, 6} and {c["instance_border_width"] for c in sc.CASES} >= {0, 1, 3}
    assert {c["instance_border_object"] for c in sc.CASES if c["n"] > 1 and c["instance_border_width"]} == {"wall", "empty"}
    kinds = {type(c["agents"]) for c in sc.CASES}
    assert kinds == {int, dict, tuple}
    assert {int(s) for s in sc.SEEDS[:4]} == {0, 1, 2 ** 31, 2 ** 32 - 1} and np.array_equal(sc.SEEDS, mc.SEEDS)


@pytest.mark.parametrize("name", ALL)
def test_spec_from_config_builds_the_references_grid(name):
    """(a) cell for cell, the full 24-agent arena included."""
    grids, configs = sc.fixture()
    spec = spec_from_config(configs[name])
    want = sc.spec_of(name)
    assert isinstance(spec, MapGenSpec) and vars(spec) == vars(want)
    c = sc.BY_NAME[name]
    assert spec.instances_count == c["n"]
    seeds = [s for (n, s) in grids if n == name]
    assert sorted(seeds) == sorted(sc.FIXTURE_SEEDS)
    for seed in seeds:
        got, ref = spec.random_map(seed), grids[(name, seed)]
        assert got.shape == ref.shape == (spec.map_height, spec.map_width) and (got == ref).all(), (name, seed)


def test_spec_from_config_random_builder():
    d = {"type": "mettagrid.map_builder.random_map.RandomMapBuilder.Config", "seed": 7, "width": 14, "height": 11,
         "objects": {"wall": 12}, "agents": 6, "border_width": 0, "border_object": "wall"}
    spec = spec_from_config(d)
    assert isinstance(spec, RandomMapSpec)
    assert (spec.random_map(7) == mapgen.random_map(11, 14, {"wall": 12}, 6, 7, 0)).all()


def _config():
    return copy.deepcopy(sc.fixture()[1]["arena_4x4"])


@pytest.mark.parametrize("field,change", [
    ("type", lambda d: d.update(type="mettagrid.map_builder.ascii.AsciiMapBuilder.Config")),
    ("instance.type", lambda d: d["instance"].update(type="mettagrid.mapgen.scenes.maze.Maze.Config")),
    ("instance", lambda d: d.update(instance={"type": "mettagrid.map_builder.random_map.RandomMapBuilder.Config", "width": 3, "height": 3})),
    ("instance", lambda d: d.update(instance={"type": "mettagrid.mapgen.mapgen.MapGen.Config"})),
    ("instance.children", lambda d: d["instance"].update(children=[{"scene": {}, "where": "full"}])),
    ("instance.transform", lambda d: d["instance"].update(transform="rot_90")),
    ("instance.seed", lambda d: d["instance"].update(seed=3)),
    ("instance_border_clear_radius", lambda d: d.update(instance_border_clear_radius=1)),
    ("instance_object_remap", lambda d: d.update(instance_object_remap={"hub": "hub_{instance_id}"})),
    ("instance_names", lambda d: d.update(instance_names=["a", "b", "c", "d"])),
])
def test_spec_from_config_refuses_naming_the_field(field, change):
    d = _config()
    assert isinstance(spec_from_config(d), MapGenSpec)
    change(d)
    with pytest.raises(UnsupportedMapBuilder, match=f"'{field}'"):
        spec_from_config(d)
    assert issubclass(UnsupportedMapBuilder, ValueError)


@pytest.mark.parametrize("name", NAMES)
def test_generated_class_maps_equals_the_string_maps(name):
    """(b) the vectorised restatement (own SeedSequence, PCG64, two shuffles on one stream) against numpy's generators."""
    prog, spec = sc.case(name)
    got = generated_class_maps(spec, prog, sc.SEEDS)
    assert got.dtype == np.uint16 and got.shape == (len(sc.SEEDS), spec.map_height, spec.map_width)
    for i, s in enumerate(sc.SEEDS):
        assert np.array_equal(got[i], prog.class_map(spec.random_map(int(s)))), (name, int(s))
    grids, _ = sc.fixture()
    for seed in sc.FIXTURE_SEEDS:
        assert np.array_equal(generated_class_maps(spec, prog, [seed])[0], prog.class_map(grids[(name, seed)])), (name, seed)


@pytest.mark.parametrize("key", [0, 1, 2, 15])
def test_seedseq_pool_with_a_spawn_key(key):
    """(c)"""
    with np.errstate(over="ignore"):
        got = np.stack(er.generate_state8(er.seedseq_pool(sc.SEEDS, key)), axis=1).astype(np.uint32)
        plain = np.stack(er.generate_state8(er.seedseq_pool(sc.SEEDS)), axis=1).astype(np.uint32)
    for i, s in enumerate(sc.SEEDS):
        assert np.array_equal(got[i], np.random.SeedSequence(int(s), spawn_key=(key,)).generate_state(8, np.uint32)), (int(s), key)
        assert np.array_equal(plain[i], np.random.SeedSequence(int(s)).generate_state(8, np.uint32))
        child = np.random.SeedSequence(int(s)).spawn(key + 1)[key]
        assert np.array_equal(got[i], child.generate_state(8, np.uint32))


def test_two_shuffles_on_one_stream():
    base, then = np.arange(7, dtype=np.uint16), np.arange(130, dtype=np.int64)
    a, b = mapgen.shuffled_rows(base, sc.SEEDS, then=then, key=3)
    for i, s in enumerate(sc.SEEDS):
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(s), spawn_key=(3,))))
        x, y = base.copy(), then.copy()
        rng.shuffle(x)
        rng.shuffle(y)
        assert np.array_equal(a[i], x) and np.array_equal(b[i], y)


def test_lower_refuses_what_it_must():
    """(d)"""
    prog, spec = sc.case("arena_4x4")
    low = spec.lower(prog)
    assert (low.n_inst, low.rows, low.cols, low.first_on_root) == (4, 2, 2, True) and low.symbols.shape == (4, 14)
    assert (spec.instances_count, spec.map_height, spec.map_width) == (4, 62, 62)
    kw = sc.spec_kwargs(sc.BY_NAME["arena_4x4"])
    with pytest.raises(ValueError, match="program's map is 62 x 62"):
        MapGenSpec(**{**kw, "border_width": 5}).lower(prog)
    with pytest.raises(ValueError, match="not divisible"):
        MapGenSpec(**{**kw, "num_agents": 15}).lower(prog)
    with pytest.raises(ValueError, match="instances asks for 3"):
        MapGenSpec(**{**kw, "instances": 3}).lower(prog)
    with pytest.raises(ValueError, match="do not fit the 625 cells of a room"):
        MapGenSpec(**{**kw, "objects": {"wall": 622}}).lower(prog)
    with pytest.raises(ValueError, match="more 'agent.agent' cells than agents"):
        MapGenSpec(**{**kw, "agents": 5, "num_agents": 20}).lower(prog)
    with pytest.raises(ValueError, match="the reference cannot build this map"):
        MapGenSpec(3, 3, {}, 1, instances=1, border_width=0).random_map(0)
    keyed = sc.case("n3_keyed")
    lk = keyed[1].lower(keyed[0])
    assert not lk.first_on_root and lk.n_teams == 3 and len({tuple(r) for r in lk.symbols.tolist()}) == 3
    assert not sc.case("n1_teams_keyed")[1].first_on_root and sc.case("n1_teams_root")[1].first_on_root

    class Far:   # a program whose class ids reach the team codes
        words = prog.words
        agent_rename = prog.agent_rename
        cell_to_class = {**prog.cell_to_class, "wall": mapgen.TEAM0}
    with pytest.raises(ValueError, match="class ids reach the team codes"):
        spec.lower(Far)

    class Crowd:   # ... with more agent groups than team codes
        words = prog.words
        cell_to_class = prog.cell_to_class
        agent_rename = {f"agent.team_{k}": [k, k] for k in range(mapgen.MAX_TEAMS + 1)}
    many = MapGenSpec(1, 2, {}, 2, instances=mapgen.MAX_TEAMS + 1, border_width=1, instance_border_width=0, set_team_by_instance=True)

    class CrowdProg(Crowd):
        words = np.array([0, 0, 0, many.map_height, many.map_width], np.int64)
    with pytest.raises(ValueError, match="more than 256 agent teams"):
        many.lower(CrowdProg)


def test_random_map_spec_results_are_unchanged():
    """(d) the random builder's host path after the shuffle was factored into a stream object: numpy's own shuffles."""
    for a, seed, perm in mc.fixture():
        got = mapgen.shuffled_rows(np.arange(a, dtype=np.uint16), [seed])
        assert np.array_equal(got[0], perm), (a, seed)
    prog, spec = mc.case(129, 1, True)
    assert np.array_equal(generated_class_maps(spec, prog, mc.SEEDS[:6]),
                          np.stack([prog.class_map(spec.random_map(int(s))) for s in mc.SEEDS[:6]]))
