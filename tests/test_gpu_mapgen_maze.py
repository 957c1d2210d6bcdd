"""GPU: the maze recipe of the device map generator (include/mgx.h mgx_set_map_maze_generator; csrc/mgx_mapgen.h mgx_maze_kernel)
against its host restatement (mapgen.generated_class_maps, itself checked against numpy and the reference's grids in
tests/test_mapgen_maze_host.py) and against the reference's grids, as the map source of host-driven restarts and of on-device
auto-reset, and beside the two other recipe kinds in one engine."""
import os

import numpy as np
import pytest

import maze_cases as zc
from mettagrid_amd import presets
from mettagrid_amd.engine import BatchedMettaGrid, MgxError
from mettagrid_amd.mapgen import LoweredMaze, MapGenSpec, MazeGenSpec, RandomMapSpec, generated_class_maps
from test_gpu_mapgen import _wrapper_pair

pytestmark = pytest.mark.gpu


def _create_map(prog, spec):
    """A map to create an engine with: one of the recipe's, or — for a recipe that places no agent — of the same geometry
    with one (no env is ever built from the agent-less maps; generate_maps touches none)."""
    if isinstance(spec, MazeGenSpec) and not spec.instance_symbols(0):
        spec = MazeGenSpec(spec.width, spec.height, {}, 1, instances=spec.instances, border_width=spec.border_width,
                           instance_border_width=spec.instance_border_width, algorithm=spec.algorithm, room_size=spec.room_size,
                           wall_size=spec.wall_size)
    return generated_class_maps(spec, prog, [0])


def _engine(prog, spec, E=1, base=0):
    one = _create_map(prog, spec)
    eng = BatchedMettaGrid(prog, np.broadcast_to(one, (E,) + one.shape[1:]), np.arange(E, dtype=np.uint32), buffers="device")
    eng.set_map_generator(spec, base)
    return eng


@pytest.mark.parametrize("name", zc.NAMES)
def test_generate_maps_equals_the_host_maps(name):
    """One launch of mixed seeds per case; the reference's own grids for the fixture seeds."""
    prog, spec = zc.case(name)
    eng = _engine(prog, spec)
    got = eng.generate_maps(zc.SEEDS)
    assert got.dtype == np.uint16 and np.array_equal(got, generated_class_maps(spec, prog, zc.SEEDS))
    grids, _ = zc.fixture()
    ref = np.stack([prog.class_map(grids[(name, s)]) for s in zc.FIXTURE_SEEDS])
    assert np.array_equal(eng.generate_maps(list(zc.FIXTURE_SEEDS)), ref)
    eng.close()


@pytest.mark.parametrize("name", ["r17x17_kruskal", "r10x13_ws2_dfs"])
def test_generate_maps_into_device_memory(name):
    import torch
    prog, spec = zc.case(name)
    eng = _engine(prog, spec)
    out = torch.zeros((len(zc.SEEDS), spec.map_height, spec.map_width), dtype=torch.int16, device="cuda")
    eng.generate_maps(zc.SEEDS, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), generated_class_maps(spec, prog, zc.SEEDS))
    eng.close()


def _maze4(algorithm, max_steps=0):
    """A 4-instance maze recipe (9 x 9 rooms, border 1, {"wall": 3, "chest": 1}) on the rung-3 preset's rules: 4 x (2 red + 2 blue)."""
    spec = MazeGenSpec(9, 9, {"wall": 3, "chest": 1}, {"red": 2, "blue": 2}, num_agents=16, border_width=1, instance_border_width=1,
                       algorithm=algorithm)
    rules = dict(max_steps=max_steps, episode_truncates=True) if max_steps else {}
    return zc.program(spec, list(presets.rung3_spec().agents), **rules), spec


@pytest.mark.parametrize("algorithm", ["kruskal", "dfs"])
def test_reset_envs_generated_equals_a_fresh_engine(algorithm):
    """Masked restarts on generated maps = a fresh engine on the host maps of the same seeds; the others are untouched."""
    import torch
    prog, spec = _maze4(algorithm)
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
    """96 envs, the 4-instance maze recipe on rung-3 rules, max_steps 11, desync, 60 steps; a base near 2**32 so that seeds wrap."""
    prog, spec = _maze4("dfs", max_steps=11)
    ep = _wrapper_pair(prog, spec, 96, 60, map_seed=2 ** 32 - 40, stride=1)
    assert ep.min() >= 4


def _lowered_with(low, **changes) -> LoweredMaze:
    kw = dict(height=low.height, width=low.width, room_height=low.room_height, room_width=low.room_width, n_inst=low.n_inst, rows=low.rows,
              cols=low.cols, border_width=low.border_width, instance_border_width=low.instance_border_width, border_code=low.border_code,
              instance_border_code=low.instance_border_code, first_on_root=low.first_on_root, key_offset=low.key_offset,
              algorithm=low.algorithm, room_size=low.room_size, wall_size=low.wall_size, wall_code=low.wall_code, n_empty=low.n_empty,
              symbols=low.symbols.copy(), rename=low.rename, rename_off=low.rename_off)
    kw.update(changes)
    return LoweredMaze(**kw)


def _lds_bytes(spec) -> int:
    """What the maze kernel needs (csrc/mgx_mapgen.h MGX_MAZE_LDS_BYTES): map, max(walls, cells), cells, room area, symbols; 2 B each."""
    from mettagrid_amd.mapgen import maze_geometry
    _, _, cols, rows = maze_geometry(spec.height, spec.width, spec.room_size, spec.wall_size)
    words = (spec.map_height * spec.map_width + max(spec.n_walls, cols * rows) + cols * rows + spec.height * spec.width +
             len(spec.instance_symbols(0)))
    return (words * 2 + 15) & ~15


def test_one_engine_changes_recipes_and_refusals_keep_the_recipe_that_is_set():
    """random -> scene -> maze -> random -> off, each recipe generating its own maps; a refused maze recipe (too many symbols, bad
    geometry, a class id past the program's, too little LDS) leaves the engine generating the previous recipe's maps with the
    previous base seeds."""
    prog, maze = _maze4("kruskal")
    other = _maze4("dfs")[1]
    H, W = maze.map_height, maze.map_width
    rand = RandomMapSpec(H, W, {"wall": 20, "extractor": 6, "chest": 3}, {"red": 8, "blue": 8})
    scene = MapGenSpec(9, 9, {"wall": 3, "chest": 1}, {"red": 2, "blue": 2}, num_agents=16, border_width=1, instance_border_width=1)
    assert (scene.map_height, scene.map_width) == (H, W) == (21, 21)
    eng = _engine(prog, rand, 2, [5, 6])
    seeds = [123, 2 ** 32 - 1]
    need = _lds_bytes(maze)
    assert need == 2 * (441 + 40 + 25 + 81 + 8) + 10   # 1 190 B, rounded up to a multiple of 16

    def generates(spec, base):
        assert np.array_equal(eng.generate_maps(seeds), generated_class_maps(spec, prog, seeds)) and np.array_equal(eng.map_seeds(), base)

    def refusals(spec, base):
        low = maze.lower(prog)
        assert low.n_empty == 49 and low.n_sym == 8
        crowded = _lowered_with(low, symbols=np.full((4, 50), low.wall_code, np.uint16))
        with pytest.raises(ValueError, match="50 symbols do not fit the 49 empty cells"):
            eng.set_map_generator(crowded, [1, 2])
        generates(spec, base)
        with pytest.raises(ValueError, match="must add up to the program's"):
            eng.set_map_generator(_lowered_with(low, border_width=2), [1, 2])
        generates(spec, base)
        with pytest.raises(ValueError, match="neither kruskal"):
            eng.set_map_generator(_lowered_with(low, algorithm=2), [1, 2])
        generates(spec, base)
        bad = _lowered_with(low)
        bad.symbols[3, 0] = 4000   # a class id past the program's
        with pytest.raises(ValueError, match="class map holds id 4000"):
            eng.set_map_generator(bad, [1, 2])
        generates(spec, base)
        with pytest.raises(ValueError, match="class map holds id 4001"):
            eng.set_map_generator(_lowered_with(low, wall_code=4001), [1, 2])
        generates(spec, base)
        os.environ["MGX_MAPGEN_LDS_BYTES"] = str(need - 16)
        try:
            with pytest.raises(MgxError, match="LDS"):
                eng.set_map_generator(maze, [1, 2])
        finally:
            del os.environ["MGX_MAPGEN_LDS_BYTES"]
        generates(spec, base)

    generates(rand, [5, 6])
    refusals(rand, [5, 6])
    eng.set_map_generator(scene, [7, 8])
    generates(scene, [7, 8])
    refusals(scene, [7, 8])
    os.environ["MGX_MAPGEN_LDS_BYTES"] = str(need)   # exactly what the maze recipe needs
    try:
        eng.set_map_generator(maze, [9, 10])
    finally:
        del os.environ["MGX_MAPGEN_LDS_BYTES"]
    generates(maze, [9, 10])
    refusals(maze, [9, 10])
    eng.set_map_generator(other, [11, 12])   # one maze recipe replaces another
    generates(other, [11, 12])
    eng.set_map_generator(rand, [13, 14])
    generates(rand, [13, 14])
    eng.set_map_generator(maze, [15, 16])
    # the generator cannot go while it is auto-reset's map source, whichever recipe it holds
    eng.set_auto_reset(True)
    with pytest.raises(ValueError, match="map source of auto-reset"):
        eng.set_map_generator(None)
    generates(maze, [15, 16])
    eng.set_auto_reset(False)
    eng.set_map_generator(None)
    with pytest.raises(ValueError, match="no map generator"):
        eng.generate_maps(seeds)
    eng.close()


def test_a_set_generator_alone_enqueues_nothing():
    """Two engines stepped alike, one with a maze generator set and never used for a restart: equal state digests and observations."""
    import torch
    prog, spec = _maze4("dfs")
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
