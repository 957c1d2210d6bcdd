"""GPU: the device map generator (include/mgx.h mgx_set_map_generator; csrc/mgx_mapgen.h) against its host restatement
(mapgen.generated_class_maps, itself checked against numpy in tests/test_mapgen_device.py), as the map source of host-driven
restarts and of on-device auto-reset."""
import os

import numpy as np
import pytest

import mapgen_cases as mc
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid, MgxError
from mettagrid_amd.envs import MettaGridBatchedEnv
from mettagrid_amd.mapgen import RandomMapSpec, generated_class_maps

pytestmark = pytest.mark.gpu

R3_OBJECTS = {"wall": 20, "extractor": 6, "chest": 3}
R3_AGENTS = {"red": 8, "blue": 8}


def _engine(prog, spec, E=1, base=0, buffers="device"):
    one = generated_class_maps(spec, prog, [0])
    eng = BatchedMettaGrid(prog, np.broadcast_to(one, (E,) + one.shape[1:]), np.arange(E, dtype=np.uint32), buffers=buffers)
    eng.set_map_generator(spec, base)
    return eng


@pytest.mark.parametrize("two_teams", [False, True])
@pytest.mark.parametrize("border", mc.BORDERS)
@pytest.mark.parametrize("area", mc.AREAS)
def test_generate_maps_equals_the_host_maps(area, border, two_teams):
    """(e) one launch of mixed seeds per shape; (f) the committed numpy shuffles of that area."""
    prog, spec = mc.case(area, border, two_teams)
    eng = _engine(prog, spec)
    got = eng.generate_maps(mc.SEEDS)
    assert got.dtype == np.uint16 and np.array_equal(got, generated_class_maps(spec, prog, mc.SEEDS))
    low = spec.lower(prog)
    for a, seed, perm in mc.fixture():
        if a == area:
            assert np.array_equal(eng.generate_maps([seed])[0], mc.maps_from_perm(low, perm)), (area, seed)
    eng.close()


def test_generate_maps_into_device_memory():
    import torch
    prog, spec = mc.case(900, 1, True)
    eng = _engine(prog, spec)
    out = torch.zeros((len(mc.SEEDS), spec.height, spec.width), dtype=torch.int16, device="cuda")
    eng.generate_maps(mc.SEEDS, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), generated_class_maps(spec, prog, mc.SEEDS))
    eng.close()


def _r3(H=16, W=16, max_steps=0):
    spec = presets.rung3_spec()
    if max_steps:
        spec.max_steps = max_steps
        spec.episode_truncates = True
    prog = compile_spec(spec, H, W, max_objects=192)
    return prog, RandomMapSpec(H, W, R3_OBJECTS, R3_AGENTS)


def test_reset_envs_generated_equals_a_fresh_engine():
    """(g) masked restarts on generated maps = a fresh engine on the host maps of the same seeds; the others are untouched."""
    prog, spec = _r3()
    E, A = 12, prog.num_agents
    base = 1000 + 7 * np.arange(E, dtype=np.uint32)
    eng = _engine(prog, spec, E, base)
    import torch
    rng = np.random.RandomState(3)
    for _ in range(5):
        eng.actions.copy_(torch.as_tensor(rng.randint(0, len(prog.action_names), E * A).astype(np.int32)).cuda())
        torch.cuda.synchronize()
        eng.step()
    eng.sync()
    before_d, before_o = eng.state_digests(), eng.obs.cpu().numpy().copy()
    mask = np.zeros(E, np.uint8)
    mask[[0, 3, 4, 11]] = 1
    explicit = (4000000000 + np.arange(E)).astype(np.uint32)
    for map_seeds in (None, explicit):
        eng.reset_envs_generated(mask, map_seeds)
        want_seeds = base if map_seeds is None else explicit
        fresh = BatchedMettaGrid(prog, generated_class_maps(spec, prog, want_seeds), np.arange(E, dtype=np.uint32), buffers="device")
        fd, fo = fresh.state_digests(), fresh.obs.cpu().numpy()
        d, o = eng.state_digests(), eng.obs.cpu().numpy()
        m = mask.astype(bool)
        assert np.array_equal(d[m], fd[m]) and np.array_equal(o.reshape(E, A, -1)[m], fo.reshape(E, A, -1)[m])
        assert np.array_equal(d[~m], before_d[~m]) and np.array_equal(o.reshape(E, A, -1)[~m], before_o.reshape(E, A, -1)[~m])
        assert np.array_equal(eng.map_seeds()[m], want_seeds[m]) and np.array_equal(eng.map_seeds()[~m], base[~m])
        fresh.close()
    eng.close()


def _wrapper_pair(prog, spec, E, steps, map_seed, stride):
    """Steps the wrapper in map_gen mode and in map_fn mode (host maps of seed base[e] + k) with the same actions.  map_fn mode
    has no desync of its own: the test plays EarlyResetHandler for it (truncations set once step >= the drawn step in an env's
    first episode), which is what the device does in auto-reset mode.  The episode counter of a record is only kept on the
    device in auto-reset mode, so the infos are compared without it."""
    import torch
    A = prog.num_agents
    gen = MettaGridBatchedEnv(prog, E, map_gen=spec, map_seed=map_seed, map_seed_stride=stride, desync=True, seed=5, episode_log=4096)
    base = gen.map_seed_bases()
    K = 12   # more episodes than an env can play here; all host maps at once
    table = generated_class_maps(spec, prog, ((base.astype(np.int64)[:, None] + np.arange(K)) & 0xFFFFFFFF).reshape(-1))
    fn = MettaGridBatchedEnv(prog, E, map_fn=lambda e, k: table[e * K + k], seed=5, episode_log=4096)
    og, _ = gen.reset()
    of, _ = fn.reset()
    early = torch.as_tensor(fn.early_end_steps().astype(np.int64), device="cuda")
    assert torch.equal(og, of)
    rng = np.random.RandomState(11)
    n_act = gen.transport_action_n
    for t in range(steps):
        a = torch.as_tensor(rng.randint(0, n_act, E * A).astype(np.int32), device="cuda")
        rg = gen.step(a)
        rf = fn.step(a)
        cur = torch.as_tensor(fn.engine.current_steps().astype(np.int64), device="cuda")
        first = torch.as_tensor(fn.episode == 0, device="cuda")
        hit = first & (early > 0) & (cur >= early)
        fn.engine.truncations.view(E, A)[hit] = 1
        for k, name in enumerate(("observations", "rewards", "terminals", "truncations")):
            assert torch.equal(rg[k], rf[k]), (t, name)
    ep, _ = gen.engine.episodes()
    assert np.array_equal(ep, fn.episode)
    done = fn._done_envs()   # (map_fn mode records an env when it restarts it: the ones the last step finished are still open)
    if done.any():
        fn.engine.record_episodes(done)
    assert np.array_equal(gen.engine.map_seeds(), ((base.astype(np.int64) + ep) & 0xFFFFFFFF).astype(np.uint32))
    ig, jf = gen.episode_infos(), fn.episode_infos()
    key = lambda r: (r["env"], r["attributes"]["steps"], tuple(r["episode_rewards"]))
    assert len(ig) == len(jf) and gen.episodes_dropped == 0
    by_env = {}
    for r in ig:   # the records of an env count its episodes 0, 1, 2 ... and name no pool map
        assert r["episode"] == by_env.get(r["env"], 0) and r["map_index"] == -1
        by_env[r["env"]] = r["episode"] + 1
    strip = lambda r: {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != "episode"}
    assert [strip(r) for r in sorted(ig, key=key)] == [strip(r) for r in sorted(jf, key=key)]
    gen.close()
    fn.close()
    return ep


def test_wrapper_map_gen_equals_map_fn_rung3():
    """(h) 96 envs, rung-3 rules, max_steps 11, desync, 60 steps; a base near 2**32 so that seeds wrap."""
    prog, spec = _r3(max_steps=11)
    ep = _wrapper_pair(prog, spec, 96, 60, map_seed=2 ** 32 - 40, stride=1)
    assert ep.min() >= 4


def test_wrapper_map_gen_equals_map_fn_rung4():
    """(i) the rung-4 preset's rules at 8 envs: extended construction, AoE and territory sources from generated maps."""
    spec4 = presets.rung4_spec()
    spec4.max_steps = 11
    spec4.episode_truncates = True
    H = W = 64
    prog = compile_spec(spec4, H, W, max_objects=presets.RUNG4_MAX_OBJECTS)
    spec = RandomMapSpec(H, W, dict(presets.RUNG4_OBJECTS), dict(presets.RUNG4_AGENTS))
    ep = _wrapper_pair(prog, spec, 8, 60, map_seed=77, stride=1 << 16)
    assert ep.min() >= 4


def test_a_forked_env_takes_the_destination_slots_next_map():
    """(j) env 3 saved and loaded onto env 40: both finish the episode alike; env 40's next map is the host map of
    base[40] + the moved episode count."""
    import torch
    prog, spec = _r3(max_steps=7)
    E, A = 48, prog.num_agents
    env = MettaGridBatchedEnv(prog, E, map_gen=spec, map_seed=9, map_seed_stride=1000, seed=2)
    env.reset()
    base = env.map_seed_bases()
    zeros = torch.zeros(E * A, dtype=torch.int32, device="cuda")
    for _ in range(9):   # into the second episode
        env.step(zeros)
    env.load_state(env.save_state([3]), [40])
    ep, _ = env.engine.episodes()
    assert ep[3] == ep[40] == 1
    for _ in range(7):   # past the next restart of both
        env.step(zeros)
    ep2, _ = env.engine.episodes()
    assert ep2[3] == ep2[40] == 2
    seeds = env.engine.map_seeds()
    assert seeds[40] == base[40] + 2 and seeds[3] == base[3] + 2
    maps = generated_class_maps(spec, prog, [seeds[3], seeds[40]])
    fresh = BatchedMettaGrid(prog, maps, env._seeds()[[3, 40]], buffers="device")
    for _ in range(2):   # both restarted two steps ago (lazy auto-reset: restart, then the step)
        fresh.step()
    fresh.sync()
    assert np.array_equal(env.engine.state_digests()[[3, 40]], fresh.state_digests())
    fresh.close()
    env.close()


def test_refusals_leave_the_engine_as_it_was():
    """(k)"""
    from mettagrid_amd import mapgen
    prog, spec = _r3()
    eng = _engine(prog, spec, 2, [5, 6])
    want = generated_class_maps(spec, prog, [123])

    def still_set():
        assert np.array_equal(eng.generate_maps([123]), want) and np.array_equal(eng.map_seeds(), [5, 6])

    low = spec.lower(prog)
    bad = mapgen.LoweredMap(low.height, low.width, low.border_width, low.border_code, low.inner.copy(), low.rename, low.rename_off)
    bad.inner[0] = 4000   # a class id past the program's
    with pytest.raises(ValueError, match="class map holds id"):
        eng.set_map_generator(bad, [1, 2])
    still_set()
    os.environ["MGX_MAPGEN_LDS_BYTES"] = "256"   # the inner area (14 x 14 x 2 B) does not fit that workgroup
    try:
        with pytest.raises(MgxError, match="LDS"):
            eng.set_map_generator(spec, [1, 2])
    finally:
        del os.environ["MGX_MAPGEN_LDS_BYTES"]
    still_set()
    os.environ["MGX_MAPGEN_LDS_BYTES"] = "64k"   # the test hook takes a decimal byte count and nothing else
    try:
        with pytest.raises(ValueError, match="not a decimal byte count"):
            eng.set_map_generator(spec, [1, 2])
    finally:
        del os.environ["MGX_MAPGEN_LDS_BYTES"]
    still_set()
    # the generator cannot go while it is auto-reset's map source (finished envs would be rebuilt from stale maps)
    eng.set_auto_reset(True)
    with pytest.raises(ValueError, match="map source of auto-reset"):
        eng.set_map_generator(None)
    still_set()
    eng.set_auto_reset(False)
    eng.close()
    # neither pool nor generator: today's error
    one = generated_class_maps(spec, prog, [0])
    eng = BatchedMettaGrid(prog, one, [0], buffers="device")
    with pytest.raises(ValueError, match=r"mgx_set_auto_reset: no map pool \(mgx_set_map_pool\)"):
        eng.set_auto_reset(True)
    eng.set_map_generator(spec, [1])
    eng.set_auto_reset(True)
    eng.set_auto_reset(False)
    eng.set_map_generator(None)
    with pytest.raises(ValueError, match=r"mgx_set_auto_reset: no map pool \(mgx_set_map_pool\)"):
        eng.set_auto_reset(True)
    eng.close()


def test_a_recipe_with_more_aoe_sources_than_the_create_maps_is_refused():
    """(k) capacities are sized from the create maps; a recipe that places more sources is refused whole."""
    spec4 = presets.rung4_spec()
    H = W = 64
    prog = compile_spec(spec4, H, W, max_objects=presets.RUNG4_MAX_OBJECTS)
    small = RandomMapSpec(H, W, dict(presets.RUNG4_OBJECTS), dict(presets.RUNG4_AGENTS))
    eng = _engine(prog, small, 1, [3])
    more = dict(presets.RUNG4_OBJECTS)
    for k in more:
        if k != "wall":
            more[k] += 3
    with pytest.raises(MgxError, match="more AoE / territory sources"):
        eng.set_map_generator(RandomMapSpec(H, W, more, dict(presets.RUNG4_AGENTS)), [9])
    assert np.array_equal(eng.generate_maps([8]), generated_class_maps(small, prog, [8])) and eng.map_seeds()[0] == 3
    eng.close()
