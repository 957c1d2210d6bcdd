"""GPU: the scene recipe of the device map generator (include/mgx.h mgx_set_map_scene_generator; csrc/mgx_mapgen.h
mgx_mapscene_kernel) against its host restatement (mapgen.generated_class_maps, itself checked against numpy and the reference's
grids in tests/test_mapgen_scene_host.py), as the map source of host-driven restarts and of on-device auto-reset, and beside
the random-builder recipe in one engine."""
import os

import numpy as np
import pytest

import mapgen_scene_cases as sc
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid, MgxError
from mettagrid_amd.mapgen import LoweredScene, MapGenSpec, RandomMapSpec, generated_class_maps
from test_gpu_mapgen import _wrapper_pair

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in sc.CASES]


def _create_map(prog, spec):
    """A map to create an engine with: one of the recipe's, or — for a recipe that places no agent — of the same geometry
    with one (no env is ever built from the agent-less maps; generate_maps touches none)."""
    if isinstance(spec, MapGenSpec) and not spec.instance_symbols(0):
        spec = MapGenSpec(spec.width, spec.height, {}, 1, instances=spec.instances, border_width=spec.border_width,
                          instance_border_width=spec.instance_border_width)
    return generated_class_maps(spec, prog, [0])


def _engine(prog, spec, E=1, base=0):
    one = _create_map(prog, spec)
    eng = BatchedMettaGrid(prog, np.broadcast_to(one, (E,) + one.shape[1:]), np.arange(E, dtype=np.uint32), buffers="device")
    eng.set_map_generator(spec, base)
    return eng


@pytest.mark.parametrize("name", NAMES)
def test_generate_maps_equals_the_host_maps(name):
    """(e) one launch of mixed seeds per case; the reference's own grids for the fixture seeds."""
    prog, spec = sc.case(name)
    eng = _engine(prog, spec)
    got = eng.generate_maps(sc.SEEDS)
    assert got.dtype == np.uint16 and np.array_equal(got, generated_class_maps(spec, prog, sc.SEEDS))
    grids, _ = sc.fixture()
    ref = np.stack([prog.class_map(grids[(name, s)]) for s in sc.FIXTURE_SEEDS])
    assert np.array_equal(eng.generate_maps(list(sc.FIXTURE_SEEDS)), ref)
    eng.close()


def test_generate_maps_into_device_memory():
    import torch
    prog, spec = sc.case("arena_4x4_keyed")
    eng = _engine(prog, spec)
    out = torch.zeros((len(sc.SEEDS), spec.map_height, spec.map_width), dtype=torch.int16, device="cuda")
    eng.generate_maps(sc.SEEDS, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), generated_class_maps(spec, prog, sc.SEEDS))
    eng.close()


def _arena(max_steps=0):
    """The 4-instance arena recipe (25 x 25 rooms, border 6, {"wall": 10}) on the rung-3 preset's rules: 4 x (2 red + 2 blue)."""
    rules = presets.rung3_spec()
    if max_steps:
        rules.max_steps = max_steps
        rules.episode_truncates = True
    spec = MapGenSpec(25, 25, {"wall": 10}, {"red": 2, "blue": 2}, num_agents=16, border_width=6, instance_border_width=0)
    return compile_spec(rules, spec.map_height, spec.map_width, max_objects=sc.object_slots(spec)), spec


def test_reset_envs_generated_equals_a_fresh_engine():
    """(f) masked restarts on generated maps = a fresh engine on the host maps of the same seeds; the others are untouched."""
    import torch
    prog, spec = _arena()
    E, A = 12, prog.num_agents
    base = 1000 + 7 * np.arange(E, dtype=np.uint32)
    eng = _engine(prog, spec, E, base)
    rng = np.random.RandomState(3)
    for _ in range(5):
        eng.actions.copy_(torch.as_tensor(rng.randint(0, len(prog.action_names), E * A).astype(np.int32)).cuda())
        torch.cuda.synchronize()
        eng.step()
    eng.sync()
    before_d, before_o = eng.state_digests(), eng.obs.cpu().numpy().copy()
    mask = np.zeros(E, np.uint8)
    mask[[0, 3, 4, 11]] = 1
    m = mask.astype(bool)
    explicit = (4000000000 + np.arange(E)).astype(np.uint32)
    for map_seeds in (None, explicit):
        eng.reset_envs_generated(mask, map_seeds)
        want_seeds = base if map_seeds is None else explicit
        fresh = BatchedMettaGrid(prog, generated_class_maps(spec, prog, want_seeds), np.arange(E, dtype=np.uint32), buffers="device")
        fd, fo = fresh.state_digests(), fresh.obs.cpu().numpy()
        d, o = eng.state_digests(), eng.obs.cpu().numpy()
        assert np.array_equal(d[m], fd[m]) and np.array_equal(o.reshape(E, A, -1)[m], fo.reshape(E, A, -1)[m])
        assert np.array_equal(d[~m], before_d[~m]) and np.array_equal(o.reshape(E, A, -1)[~m], before_o.reshape(E, A, -1)[~m])
        assert np.array_equal(eng.map_seeds()[m], want_seeds[m]) and np.array_equal(eng.map_seeds()[~m], base[~m])
        fresh.close()
    eng.close()


def test_wrapper_map_gen_equals_map_fn():
    """(g) 96 envs, the arena recipe on rung-3 rules, max_steps 11, desync, 60 steps; a base near 2**32 so that seeds wrap."""
    prog, spec = _arena(max_steps=11)
    ep = _wrapper_pair(prog, spec, 96, 60, map_seed=2 ** 32 - 40, stride=1)
    assert ep.min() >= 4


def _lowered_with(low, **changes) -> LoweredScene:
    kw = dict(height=low.height, width=low.width, room_height=low.room_height, room_width=low.room_width, n_inst=low.n_inst, rows=low.rows,
              cols=low.cols, border_width=low.border_width, instance_border_width=low.instance_border_width, border_code=low.border_code,
              instance_border_code=low.instance_border_code, first_on_root=low.first_on_root, symbols=low.symbols.copy(),
              rename=low.rename, rename_off=low.rename_off)
    kw.update(changes)
    return LoweredScene(**kw)


def test_one_engine_changes_recipes_and_refusals_keep_the_recipe_that_is_set():
    """(h) random recipe -> scene recipe -> random recipe -> off, each generating its own maps; a refused scene recipe leaves the
    engine generating the previous recipe's maps with the previous base seeds."""
    prog, scene = _arena()
    H, W = scene.map_height, scene.map_width
    rand = RandomMapSpec(H, W, {"wall": 20, "extractor": 6, "chest": 3}, {"red": 8, "blue": 8})   # (fewer cells than the arena's)
    eng = _engine(prog, rand, 2, [5, 6])
    seeds = [123, 2 ** 32 - 1]

    def generates(spec, base):
        assert np.array_equal(eng.generate_maps(seeds), generated_class_maps(spec, prog, seeds)) and np.array_equal(eng.map_seeds(), base)

    def refusals(spec, base):
        low = scene.lower(prog)
        bad = _lowered_with(low)
        bad.symbols[3, 0] = 4000   # a class id past the program's
        with pytest.raises(ValueError, match="class map holds id 4000"):
            eng.set_map_generator(bad, [1, 2])
        generates(spec, base)
        with pytest.raises(ValueError, match="class map holds id 4001"):
            eng.set_map_generator(_lowered_with(low, instance_border_code=4001), [1, 2])
        generates(spec, base)
        with pytest.raises(ValueError, match="must add up to the program's"):
            eng.set_map_generator(_lowered_with(low, border_width=5), [1, 2])
        generates(spec, base)
        os.environ["MGX_MAPGEN_LDS_BYTES"] = "8192"   # map (62 x 62) + indices (625) + symbols (14), 2 B each: 8 976 B
        try:
            with pytest.raises(MgxError, match="LDS"):
                eng.set_map_generator(scene, [1, 2])
        finally:
            del os.environ["MGX_MAPGEN_LDS_BYTES"]
        generates(spec, base)

    generates(rand, [5, 6])
    refusals(rand, [5, 6])
    eng.set_map_generator(scene, [7, 8])
    generates(scene, [7, 8])
    refusals(scene, [7, 8])
    os.environ["MGX_MAPGEN_LDS_BYTES"] = "8976"   # exactly what the scene recipe needs
    try:
        eng.set_map_generator(scene, [9, 10])
    finally:
        del os.environ["MGX_MAPGEN_LDS_BYTES"]
    generates(scene, [9, 10])
    eng.set_map_generator(rand, [11, 12])
    generates(rand, [11, 12])
    eng.set_map_generator(scene, [13, 14])
    # the generator cannot go while it is auto-reset's map source, whichever recipe it holds
    eng.set_auto_reset(True)
    with pytest.raises(ValueError, match="map source of auto-reset"):
        eng.set_map_generator(None)
    generates(scene, [13, 14])
    eng.set_auto_reset(False)
    eng.set_map_generator(None)
    with pytest.raises(ValueError, match="no map generator"):
        eng.generate_maps(seeds)
    eng.close()


def test_a_scene_recipe_with_more_aoe_sources_than_the_create_maps_is_refused():
    """(h) rung-4 rules: capacities are sized from the create maps; a recipe that places more sources is refused whole."""
    rules = presets.rung4_spec()
    objects = {k: max(1, v // 4) for k, v in presets.RUNG4_OBJECTS.items()}
    agents = {k: v // 4 for k, v in presets.RUNG4_AGENTS.items()}
    small = MapGenSpec(27, 27, objects, agents, instances=4, border_width=3, instance_border_width=4)
    assert (small.map_height, small.map_width) == (64, 64)
    prog = compile_spec(rules, 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
    eng = _engine(prog, small, 1, [3])
    more = {k: v + (1 if k != "wall" else 0) for k, v in objects.items()}
    with pytest.raises(MgxError, match="more AoE / territory sources"):
        eng.set_map_generator(MapGenSpec(27, 27, more, agents, instances=4, border_width=3, instance_border_width=4), [9])
    assert np.array_equal(eng.generate_maps([8]), generated_class_maps(small, prog, [8])) and eng.map_seeds()[0] == 3
    eng.close()


def test_a_set_generator_alone_enqueues_nothing():
    """(i) two engines stepped alike, one with a scene generator set and never used for a restart: equal state digests."""
    import torch
    prog, spec = _arena()
    E, A = 4, prog.num_agents
    maps = generated_class_maps(spec, prog, np.arange(E))
    engines = [BatchedMettaGrid(prog, maps, np.arange(E, dtype=np.uint32), buffers="device") for _ in range(2)]
    engines[1].set_map_generator(spec, 77)
    rng = np.random.RandomState(5)
    for _ in range(12):
        a = torch.as_tensor(rng.randint(0, len(prog.action_names), E * A).astype(np.int32)).cuda()
        for eng in engines:
            eng.actions.copy_(a)
        torch.cuda.synchronize()
        for eng in engines:
            eng.step()
    for eng in engines:
        eng.sync()
    assert np.array_equal(engines[0].state_digests(), engines[1].state_digests())
    assert torch.equal(engines[0].obs, engines[1].obs)
    for eng in engines:
        eng.close()
