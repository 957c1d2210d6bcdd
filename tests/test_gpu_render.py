"""GPU: rendering (mgx_render_cells / mgx_set_render_tiles / mgx_render_rgb, csrc/mgx_render.h).
Cell words against ``render.cells_from_objects(grid_objects())``, the text frame against the reference's renderer as recorded in
tests/golden/render_frames.json, RGB frames bit for bit against ``render.rgb_host`` with a random-byte atlas (a mis-indexed
texel shows), the wrappers and the refusals."""
import json
import os

import numpy as np
import pytest

import helpers as hp
import ref_tree
from mettagrid_amd import from_reference as fr
from mettagrid_amd import presets, render
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_class_maps, random_map

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "render_frames.json"), encoding="utf-8"))
R3_OBJECTS, R3_AGENTS = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}
E_RGB = 3
_engines = {}


def check_cells(eng, envs, what: str) -> np.ndarray:
    H, W = eng.map_shape
    got = eng.render_cells(envs)
    assert got.dtype == np.uint32 and got.shape == (len(envs), H, W), what
    for k, env in enumerate(envs):
        want = render.cells_from_objects(eng.prog, eng.grid_objects(int(env)), H, W)
        assert np.array_equal(got[k], want), (what, env, np.argwhere(got[k] != want)[:5])
    return got


def random_actions(prog, E: int, rng):
    n = len(prog.action_names)
    return rng.randint(0, n, E * prog.num_agents).astype(np.int32), rng.randint(0, n, E * prog.num_agents).astype(np.int32)


# ---- cells --------------------------------------------------------------------------------------------------------------------
def test_cells_torture_over_an_episode_and_a_device_restart():
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    E = 5
    maps = [hp.torture_map(s) for s in range(3)]
    prog = hp.compile_scenario("torture", hp.torture_spec(max_steps=12), *maps[0].shape)
    pool = np.stack([prog.class_map(m) for m in maps])
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=5, specialize=False, episode_stats=False)
    env.reset()
    eng = env.engine
    first = check_cells(eng, [4, 0, 2, 0], "torture reset")
    assert np.array_equal(first[1], first[3]) and (first[1] != 0).any()
    g = torch.Generator(device="cuda").manual_seed(3)
    ends, moved = 0, False
    for t in range(15):
        a = torch.randint(0, env.transport_action_n, (env.num_agents,), dtype=torch.int32, device="cuda", generator=g)
        trunc = env.step(a)[3]
        ends += int(bool(trunc.all()))
        if t in (0, 5, 10, 11, 12, 14):   # (11: the last step of the episode; 12: the first one of the restarted envs)
            moved |= not np.array_equal(check_cells(eng, [4, 0, 2, 0], f"torture step {t + 1}"), first)
    assert ends >= 1 and moved
    env.close()


def test_cells_dynamic_objects_come_and_go():
    spec_f, map_f, _, _ = hp.scenario("dynamic")
    E = 5
    maps = [map_f(s) for s in range(E)]
    prog = hp.compile_scenario("dynamic", spec_f(), *maps[0].shape)
    eng = BatchedMettaGrid(prog, np.stack([prog.class_map(m) for m in maps]), np.arange(E, dtype=np.uint32) + 11, buffers="host")
    rng = np.random.RandomState(4)
    counts = {int((check_cells(eng, [4, 0, 2, 0], "dynamic step 0") != 0).sum())}
    for t in range(24):   # the smash event fires at steps 3, 9, 20 and 21: crates go, markers come
        eng.actions[:], eng.vibe_actions[:] = random_actions(prog, E, rng)
        eng.step()
        if t + 1 in (4, 10, 22, 24):
            counts.add(int((check_cells(eng, [4, 0, 2, 0], f"dynamic step {t + 1}") != 0).sum()))
    assert eng.poll_errors()[0] == 0
    eng.close()


def reference_env(name: str, **kw):
    from mettagrid_amd.envs import MettaGridParallelEnv
    doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
    z = np.load(os.path.join(HERE, "golden", f"ref_{name}.npz"))
    cells = np.asarray(doc["map"], dtype=object)
    prog = fr.compile_reference_config(ref_tree.load(doc["config"]), *cells.shape)
    return doc, z, MettaGridParallelEnv(prog, cells, doc["seed"], **kw)


def drive(doc, z, sim, t: int) -> None:
    for when, agent_id, inv in doc["set_inventory"]:
        if when == t:
            sim.set_inventory(agent_id, dict(map(tuple, inv)))
    sim.actions()[:] = z["actions"][t]
    sim.vibe_actions()[:] = z["vibe_actions"][t]
    sim.step()


def test_cells_spawn_in_event_reference_fixture():
    doc, z, penv = reference_env("spawn_in_event")
    b = penv._sim._b
    seen = {check_cells(b, [0], "spawn_in_event step 0").tobytes()}
    for t in range(doc["steps"]):
        drive(doc, z, penv._sim, t)
        seen.add(check_cells(b, [0], f"spawn_in_event step {t + 1}").tobytes())
    assert len(seen) > 2
    penv.close()


def edge_engine():
    if "edge" not in _engines:
        prog = hp.compile_scenario("map_max_few", presets.rung3_spec(), *hp.MAP_MAX_FEW)
        cms = np.stack([prog.class_map(hp.edge_map(*hp.MAP_MAX_FEW, s)) for s in range(E_RGB)])
        _engines["edge"] = BatchedMettaGrid(prog, cms, np.arange(E_RGB, dtype=np.uint32), buffers="host", specialize=False)
    return _engines["edge"]


def test_cells_on_the_largest_map():
    eng = edge_engine()
    assert eng.map_shape == (255, 255) and eng.prog.max_objects == 64
    got = check_cells(eng, [2, 0, 2], "edge map")
    assert (got[:, 254, :] != 0).any() and (got[:, :, 254] != 0).any()


# ---- the text frame -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arena", "navigation", "spawn_in_event"])
def test_ansi_equals_the_reference_renderer(name):
    frames = {f["step"]: f for f in DOC["frames"] if f["scenario"] == name}
    assert len(frames) == 3 and 0 in frames
    doc, z, penv = reference_env(name, render_mode="ansi", render_symbols=frames[0]["symbols"])
    assert penv.render() == frames[0]["text"]
    for t in range(doc["steps"]):
        drive(doc, z, penv._sim, t)
        if t + 1 in frames:
            assert penv.render() == frames[t + 1]["text"], (name, t + 1)
    assert max(frames) == doc["steps"]
    penv.close()


# ---- RGB frames -------------------------------------------------------------------------------------------------------------------
MAPS = {"3x5": (3, 5, 4), "7x9": (7, 9, 6), "32x32": (32, 32, 16), "255x255": (255, 255, 16)}


def rgb_engine(name: str):
    """E_RGB envs of rung-3 rules (4 vibes) on the named map, stepped until agents hold vibes; shared by the cases of a map."""
    if name == "255x255":
        eng = edge_engine()
    elif name not in _engines:
        H, W, agents = MAPS[name]
        spec = hp.teams_spec(presets.rung3_spec(), agents, 2)
        if name == "32x32":
            prog = compile_spec(spec, H, W, max_objects=192)
            cms = random_class_maps(prog, H, W, R3_OBJECTS, R3_AGENTS, range(E_RGB))
        else:
            prog = compile_spec(spec, H, W)
            objects = {"wall": 2, "extractor": 1, "chest": 1} if name == "3x5" else {"wall": 8, "extractor": 3, "chest": 2}
            cms = np.stack([prog.class_map(random_map(H, W, objects, {"red": agents // 2, "blue": agents // 2}, s, border_width=0))
                            for s in range(E_RGB)])
        _engines[name] = BatchedMettaGrid(prog, cms, np.arange(E_RGB, dtype=np.uint32), buffers="host", specialize=False)
        eng = _engines[name]
    else:
        return _engines[name]
    if not getattr(eng, "_vibes_set", False):
        prog = eng.prog
        vibe_ids = [i for i, n in enumerate(prog.action_names) if n.startswith("change_vibe_")]
        assert len(vibe_ids) == 4
        eng.actions[:] = prog.action_names.index("noop")
        eng.vibe_actions[:] = [vibe_ids[k % 4] for k in range(eng.E * eng.A)]
        eng.step()
        rng = np.random.RandomState(7)
        for _ in range(2):
            eng.actions[:], eng.vibe_actions[:] = random_actions(prog, eng.E, rng)
            eng.step()
        eng._vibes_set = True
    return eng


@pytest.fixture(scope="module")
def frame_buffer():
    """An allocation of its own, 48 MiB (the caching allocator serves a request of that size with one device allocation of
    exactly that size): frames placed at its end end where the allocation ends."""
    import torch
    torch.cuda.empty_cache()
    return torch.empty(48 << 20, dtype=torch.uint8, device="cuda")


def random_atlas(prog, s: int, seed: int):
    rng = np.random.RandomState(seed)
    n_tiles = 7
    tiles = rng.randint(0, 256, (n_tiles, s, s, 3)).astype(np.uint8)
    class_tile = rng.randint(0, n_tiles, int(prog.words[render.K.H_NUM_CLASSES])).astype(np.uint16)
    agent_tile = rng.randint(0, n_tiles, prog.num_agents).astype(np.uint16)
    vibe_rgb = rng.randint(0, 256, (3, 3)).astype(np.uint8)    # vibes 1 and 2 are marked, vibe 3 is past the table
    return tiles, class_tile, agent_tile, vibe_rgb


# (envs, placement, vibe marker): placement "end" = the frames end where the allocation ends, else the byte offset from a
# 16-byte boundary: 0 -> 16-byte stores from the first byte, 4 -> dword stores in front of them, 1 -> bytes, dwords, then those
CASES = [([E_RGB - 1], "end", True), ([1, E_RGB - 1, 1], 1, True), ([E_RGB - 1], 4, False), ([0, E_RGB - 1, 0], 0, False),
         ([E_RGB - 1], 1, False), ([0, E_RGB - 1, 0], 4, True), ([E_RGB - 1], 0, True), ([1, E_RGB - 1, 1], "end", False)]
SHAPES = [(m, s) for m in MAPS for s in (1, 2, 3, 8, 16, 32) if m != "255x255" or s <= 8]


@pytest.mark.parametrize("name,s", SHAPES, ids=[f"{m}-s{s}" for m, s in SHAPES])
def test_rgb_equals_the_host_rule(name, s, frame_buffer):
    import torch
    eng = rgb_engine(name)
    H, W = eng.map_shape
    atlas = random_atlas(eng.prog, s, 100 * s + H)
    cases = CASES if name != "255x255" else CASES[:3]
    row_bytes = W * s * 3
    seen_marker = False
    for envs, place, vibe_on in cases:
        eng.set_render_tiles(*atlas[:3], atlas[3] if vibe_on else None)
        cells = eng.render_cells(envs)
        assert (cells >> 24).any(), "no agent holds a vibe: the marker is not exercised"
        want = render.rgb_host(cells, *atlas[:3], atlas[3] if vibe_on else None)
        nbytes = want.size
        assert want.shape == (len(envs), H * s, W * s, 3) and nbytes == len(envs) * H * s * row_bytes
        start = frame_buffer.numel() - nbytes if place == "end" else 4096 + place
        lo, hi = max(0, start - 64), min(frame_buffer.numel(), start + nbytes + 64)
        frame_buffer[lo:hi] = 0xA5
        torch.cuda.synchronize()
        out = frame_buffer[start:start + nbytes]
        assert place == "end" or out.data_ptr() % 16 == place
        got = eng.render_rgb(envs, out)
        eng.sync()
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == want.shape
        host = got.cpu().numpy()
        if not np.array_equal(host, want):
            bad = np.argwhere(host != want)
            raise AssertionError(f"{name} s={s} envs={envs} place={place} vibe={vibe_on}: {len(bad)} bytes differ, first at {bad[0].tolist()}")
        guard = frame_buffer[lo:hi].cpu().numpy()
        assert (guard[:start - lo] == 0xA5).all() and (guard[start - lo + nbytes:] == 0xA5).all(), "bytes outside the frames were written"
        if vibe_on and s >= 3:
            seen_marker |= not np.array_equal(want, render.rgb_host(cells, *atlas[:3], None))
    assert seen_marker or s < 3
    eng.set_render_tiles()


def test_rgb_allocates_and_repeats_a_list():
    import torch
    eng = rgb_engine("7x9")
    eng.set_render_tiles(scale=8)
    a = eng.render_rgb([2, 0])
    b = eng.render_rgb(np.array([2, 0]))      # the same list again: served from the list already on the device
    c = eng.render_rgb([0])
    eng.sync()
    assert a.dtype == torch.uint8 and tuple(a.shape) == (2, 56, 72, 3) and torch.equal(a, b) and torch.equal(c[0], a[1])
    want = render.rgb_host(eng.render_cells([2, 0]), *render.default_tiles(eng.prog, 8))
    assert np.array_equal(a.cpu().numpy(), want)
    eng.set_render_tiles()


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_frames_stay_current():
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    E, M, s = 4, 3, 4
    spec = presets.rung3_spec()
    spec.max_steps = 3
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    pool = random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(M))
    with pytest.raises(ValueError):
        MettaGridBatchedEnv(prog, E, map_pool=pool, buffers="host", render_envs=[0])
    with pytest.raises(ValueError):
        MettaGridBatchedEnv(prog, E, map_pool=pool, render_envs=[E])
    with pytest.raises(ValueError):
        MettaGridBatchedEnv(prog, E, map_pool=pool, render_envs=[0], render_scale=33)
    plain = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, specialize=False, episode_stats=False)
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, specialize=False, episode_stats=False, render_envs=[3, 0], render_scale=s)
    plain.reset(); env.reset()
    assert plain.frames is None and plain.render_mode == env.render_mode == "ansi"
    frames = env.frames
    atlas = render.default_tiles(prog, s)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 32 * s, 32 * s, 3)

    def current(what):
        assert env.frames is frames      # updated in place; read on the caller's stream, ordered by the wrapper
        want = render.rgb_host(env.engine.render_cells([3, 0]), *atlas)
        assert np.array_equal(frames.cpu().numpy(), want), what
        return want
    shown = [current("reset")]
    g = torch.Generator(device="cuda").manual_seed(1)
    ends = 0
    for t in range(4):
        a = torch.randint(0, env.transport_action_n, (env.num_agents,), dtype=torch.int32, device="cuda", generator=g)
        obs, _, _, trunc, _ = env.step(a)
        assert torch.equal(obs, plain.step(a)[0])      # the option changes nothing else
        shown.append(current(f"step {t + 1}"))
        ends += int(bool(trunc.all()))
    assert ends >= 1 and not np.array_equal(shown[0], shown[-1])
    assert np.array_equal(env.render(env=0, mode="rgb_array"), shown[-1][1])
    assert np.array_equal(plain.render(env=3, mode="rgb_array"), render.rgb_host(plain.engine.render_cells([3]), *render.default_tiles(prog, 8))[0])
    text = env.render(env=3)
    assert text == render.ansi(env.engine.render_cells([3])[0], render.class_type_names(prog)) and text.count("\n") == 31
    assert env.render(env=3, symbols={"wall": "##"}).startswith("##")
    with pytest.raises(ValueError):
        env.render(mode="human")
    st = env.save_state([0])
    env.step(torch.zeros(env.num_agents, dtype=torch.int32, device="cuda"))
    before = current("step 5")
    env.load_state(st, [3])
    after = current("load_state")
    assert np.array_equal(after[0], shown[-1][1]) and not np.array_equal(after[0], before[0])   # env 3 now shows what env 0 showed
    plain.close(); env.close()


def test_parallel_env_render_modes():
    frame0 = next(f for f in DOC["frames"] if f["scenario"] == "spawn_in_event" and f["step"] == 0)
    from mettagrid_amd.envs import MettaGridParallelEnv
    doc, z, penv = reference_env("spawn_in_event")
    assert penv.render_mode is None and penv.render() is None
    penv.close()
    doc, z, penv = reference_env("spawn_in_event", render_mode="ansi")
    assert penv.render() == frame0["text"]
    penv.reset()
    assert penv.render() == frame0["text"]
    penv.close()
    doc, z, penv = reference_env("spawn_in_event", render_mode="rgb_array", render_scale=5)
    b = penv._sim._b
    rgb = penv.render()
    H, W = b.map_shape
    assert isinstance(rgb, np.ndarray) and rgb.dtype == np.uint8 and rgb.shape == (H * 5, W * 5, 3)
    assert np.array_equal(rgb, render.rgb_host(b.render_cells([0])[0], *render.default_tiles(b.prog, 5)))
    drive(doc, z, penv._sim, 0)
    drive(doc, z, penv._sim, 1)
    assert not np.array_equal(penv.render(), rgb)
    penv.close()
    with pytest.raises(ValueError):
        MettaGridParallelEnv(b.prog, np.asarray(doc["map"], dtype=object), doc["seed"], render_mode="human")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    eng = rgb_engine("7x9")
    L, h = eng.L, eng.h
    H, W = eng.map_shape
    eng.set_render_tiles()
    with pytest.raises(ValueError):
        eng.render_rgb([0])                                   # no atlas
    tiles, class_tile, agent_tile, vibe_rgb = random_atlas(eng.prog, 2, 1)
    for bad in ([eng.E], [-1], [], [0.5]):
        with pytest.raises(ValueError):
            eng.render_cells(bad)
    bad_atlases = [
        dict(tiles=np.zeros((3, 0, 0, 3), np.uint8), class_tile=class_tile % 3, agent_tile=agent_tile % 3),        # tile_px 0
        dict(tiles=np.zeros((3, 33, 33, 3), np.uint8), class_tile=class_tile % 3, agent_tile=agent_tile % 3),      # tile_px 33
        dict(tiles=tiles, class_tile=np.where(np.arange(len(class_tile)) == 1, 7, class_tile), agent_tile=agent_tile),   # a tile index >= n_tiles
        dict(tiles=tiles, class_tile=class_tile, agent_tile=np.full_like(agent_tile, 7)),
        dict(tiles=tiles, class_tile=class_tile[:-1], agent_tile=agent_tile),
        dict(tiles=tiles.astype(np.int32), class_tile=class_tile, agent_tile=agent_tile),
        dict(tiles=tiles[:, :, :1], class_tile=class_tile, agent_tile=agent_tile),
        dict(tiles=tiles, class_tile=class_tile, agent_tile=agent_tile, vibe_rgb=np.zeros((0, 3), np.uint8)),
        dict(tiles=tiles, class_tile=class_tile),
        dict(tiles=tiles, class_tile=class_tile, agent_tile=agent_tile, scale=4),
    ]
    for kw in bad_atlases:
        with pytest.raises(ValueError):
            eng.set_render_tiles(**kw)
    with pytest.raises(ValueError):
        eng.render_rgb([0])                                   # ... and none of them became the atlas
    # ---- C level: MGX_ERR_BAD_ARG (-1) before anything is enqueued or changed ----
    envs = np.array([0, 2], np.int32)
    cells = np.zeros((2, H, W), np.uint32)
    one = torch.zeros(2 * H * 2 * W * 2 * 3, dtype=torch.uint8, device="cuda")
    ct, at = np.ascontiguousarray(class_tile), np.ascontiguousarray(agent_tile)
    ep, cp, fp = envs.ctypes.data, cells.ctypes.data, one.data_ptr()
    past, negative = np.array([0, eng.E], np.int32), np.array([-1], np.int32)       # (named: the pointers must stay valid)
    ct6, at6 = np.full_like(ct, 6), np.full_like(at, 6)
    assert L.mgx_render_rgb(h, ep, 2, fp) == -1               # no atlas
    for args in [(None, ep, 2, cp), (h, None, 2, cp), (h, ep, 2, None), (h, ep, 0, cp), (h, ep, -1, cp),
                 (h, past.ctypes.data, 2, cp), (h, negative.ctypes.data, 1, cp)]:
        assert L.mgx_render_cells(*args) == -1, args
    tp, ctp, atp = tiles.ctypes.data, ct.ctypes.data, at.ctypes.data
    for args in [(None, tp, 7, 2, ctp, atp, None, 0), (h, tp, 0, 2, ctp, atp, None, 0), (h, tp, 7, 0, ctp, atp, None, 0),
                 (h, tp, 7, 33, ctp, atp, None, 0), (h, tp, 7, 2, None, atp, None, 0), (h, tp, 7, 2, ctp, None, None, 0),
                 (h, tp, 6, 2, ct6.ctypes.data, atp, None, 0), (h, tp, 6, 2, ctp, at6.ctypes.data, None, 0),
                 (h, tp, 7, 2, ctp, atp, vibe_rgb.ctypes.data, 0), (h, tp, 7, 2, ctp, atp, vibe_rgb.ctypes.data, 257)]:
        assert L.mgx_set_render_tiles(*args) == -1, args
    assert L.mgx_render_rgb(h, ep, 2, fp) == -1               # still no atlas
    eng.set_render_tiles(tiles, class_tile, agent_tile, vibe_rgb)
    good = eng.render_rgb([0, 2], one)
    eng.sync()
    keep = good.clone()
    assert L.mgx_set_render_tiles(h, tp, 7, 33, ctp, atp, None, 0) == -1     # a refused atlas leaves the one in force
    for args in [(None, ep, 2, fp), (h, None, 2, fp), (h, ep, 2, None), (h, ep, 0, fp),
                 (h, past.ctypes.data, 2, fp)]:
        assert L.mgx_render_rgb(*args) == -1, args
    n = one.numel()
    bad_outs = [torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(n - 1, dtype=torch.uint8, device="cuda"),
                torch.zeros(n + 1, dtype=torch.uint8, device="cuda"), torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2], np.zeros(n, np.uint8)]
    for out in bad_outs:
        with pytest.raises(ValueError):
            eng.render_rgb([0, 2], out)
    with pytest.raises(ValueError):
        eng.render_rgb([], one)
    with pytest.raises(ValueError):
        eng.render_rgb([0, eng.E], one)
    eng.sync()
    assert torch.equal(eng.render_rgb([0, 2], one), keep)
    eng.sync()
    eng.set_render_tiles()


def teardown_module(module):
    for eng in _engines.values():
        eng.close()
    _engines.clear()
