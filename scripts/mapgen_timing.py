"""Cost of the device map generator (csrc/mgx_mapgen.h), in one process on one MI355X; variants alternate round by round, per
variant the median over the rounds with min / max and the coefficient of variation.
  gen      generate_maps of `envs` maps and of 64 maps (the latency a restart step sees) at rung-3 (32 x 32) and rung-4
           (64 x 64) size into device memory, event-timed on the engine's stream (seed upload and launch included), as ms and
           maps per second; beside it the host time of random_class_maps per map (measured on 512 maps).  For the KERNEL's own
           time run this mode under the profiler and hand the trace to the `trace` mode:
             rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/mapgen_timing.py 65536 256 5 gen
             python scripts/mapgen_timing.py 65536 256 5 trace DIR/<host>/run_kernel_trace.csv
  trace    no GPU: reads that kernel trace; the k-th mgx_mapgen_kernel dispatch is the k-th generate_maps call of `gen` (same
           envs and rounds), the first round is the warm-up.
  wrapper  MettaGridBatchedEnv's ms per step at `envs` envs, rung 3, max_steps = 128, desync=True: map_pool (16 maps) against
           map_gen, `steps` event-timed steps per round.
  scene    the scene recipe (MapGen + Random scene, mgx_mapscene_kernel): the reference arena as 1 instance (25 x 25 room, border
           6: a 37 x 37 map) and as 4 instances (a 62 x 62 map), each beside its yardstick, the random-builder kernel on a map of
           the same size with the same number of inner cells (625 / 2 500); generate_maps of `envs` and of 64 maps as in `gen`.
           Then the wrapper's ms per step with the 4-instance recipe on rung-3 rules at min(envs, 16 384) envs, map_pool (16 maps)
           against map_gen.
  all      gen, then wrapper, then scene (the default).
  maze     the maze recipe (MapGen + Maze scene with a Random child, mgx_maze_kernel; not part of `all`): 25 x 25 rooms, border 6,
           1 and 4 instances, kruskal and dfs, each beside its yardstick in the same process, the scene recipe (a Random instance)
           on rooms of the same size with the same symbols; generate_maps of `envs` and of 64 maps as in `gen`, and the ratios.
           Then the wrapper's ms per step with the 4-instance kruskal recipe on rung-3 rules at min(envs, 8 192) envs, map_pool
           (16 maps) against map_gen.
A plain `python bench.py` of this tree against its parent is run by hand, the two alternating.
Prints one JSON line.  Usage (GPU box): python scripts/mapgen_timing.py [envs] [steps] [rounds] [mode] [trace csv]"""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
mode = sys.argv[4] if len(sys.argv) > 4 else "all"
R3 = ({"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8})
GEN_ORDER = [(name, n) for name in ("rung3", "rung4") for n in (E, 64)]   # the order of generate_maps calls in a round


def stats(a, n_maps: int = 0) -> dict:
    a = np.asarray(a, dtype=np.float64)
    s = {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4),
         "cv_pct": round(float(a.std() / a.mean() * 100), 2)}
    if n_maps:
        s["maps_per_s"] = round(n_maps / (s["median"] * 1e-3))
    return s


out = {"envs": E, "steps": steps, "rounds": rounds, "mode": mode}

if mode == "trace":
    with open(sys.argv[5], newline="") as f:
        rows = [r for r in csv.DictReader(f) if "mgx_mapgen_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != (rounds + 1) * len(GEN_ORDER):
        raise SystemExit(f"{len(rows)} mgx_mapgen_kernel dispatches, expected {(rounds + 1) * len(GEN_ORDER)}: not a trace of the gen mode with these arguments")
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
    for k, (name, n) in enumerate(GEN_ORDER):
        out[f"kernel_{name}_{n}_ms"] = stats(ms[len(GEN_ORDER) + k::len(GEN_ORDER)], n)
    print(json.dumps(out), flush=True)
    sys.exit(0)

import torch  # noqa: E402

from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.engine import BatchedMettaGrid  # noqa: E402
from mettagrid_amd.envs import MettaGridBatchedEnv  # noqa: E402
from mettagrid_amd.mapgen import MapGenSpec, MazeGenSpec, RandomMapSpec, generated_class_maps, random_class_maps  # noqa: E402

spec3 = presets.rung3_spec()
spec3.max_steps = 128
spec3.episode_truncates = True
prog3 = compile_spec(spec3, 32, 32, max_objects=192)
rec3 = RandomMapSpec(32, 32, *R3)

if mode in ("gen", "all"):
    prog4 = compile_spec(presets.rung4_spec(), 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
    gens = {}
    for name, prog, rec in (("rung3", prog3, rec3),
                            ("rung4", prog4, RandomMapSpec(64, 64, dict(presets.RUNG4_OBJECTS), dict(presets.RUNG4_AGENTS)))):
        eng = BatchedMettaGrid(prog, generated_class_maps(rec, prog, [0]), [0], buffers="device", specialize=False)
        eng.set_map_generator(rec, [0])
        gens[name] = (eng, rec, prog)
    bufs = {(name, n): torch.zeros((n, gens[name][1].height, gens[name][1].width), dtype=torch.int16, device="cuda") for name, n in GEN_ORDER}
    seeds = {E: (np.arange(E, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32), 64: np.arange(64, dtype=np.uint32) + 12345}
    ms = {k: [] for k in GEN_ORDER}
    for r in range(rounds + 1):   # (round 0 warms up)
        for name, n in GEN_ORDER:
            eng = gens[name][0]
            st = eng._ext_stream()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            eng.generate_maps(seeds[n], out=bufs[(name, n)])
            t1.record(st)
            t1.synchronize()
            if r:
                ms[(name, n)].append(t0.elapsed_time(t1))
    for (name, n), v in ms.items():
        out[f"generate_{name}_{n}_ms"] = stats(v, n)
    for name, (eng, rec, prog) in gens.items():
        t = time.perf_counter()
        random_class_maps(prog, rec.height, rec.width, rec.objects, rec.agents, range(512))
        out[f"host_random_class_maps_{name}_us_per_map"] = round((time.perf_counter() - t) / 512 * 1e6, 1)
        eng.close()
    del bufs

if mode in ("wrapper", "all"):
    pool = generated_class_maps(rec3, prog3, range(16))
    envs = {"map_pool": MettaGridBatchedEnv(prog3, E, map_pool=pool, desync=True, episode_stats=False, specialize=False),
            "map_gen": MettaGridBatchedEnv(prog3, E, map_gen=rec3, desync=True, episode_stats=False, specialize=False)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for env in envs.values():
        env.reset()
    acts = [torch.randint(0, envs["map_gen"].transport_action_n, (E * prog3.num_agents,), generator=g, device="cuda", dtype=torch.int32) for _ in range(8)]
    wms = {k: [] for k in envs}
    for r in range(rounds + 1):
        for k, env in envs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for t in range(steps):
                env.step(acts[t % 8])
            t1.record()
            t1.synchronize()
            if r:
                wms[k].append(t0.elapsed_time(t1) / steps)
    for k, v in wms.items():
        out[f"wrapper_{k}_ms_per_step"] = stats(v)
        out[f"wrapper_{k}_ms_rounds"] = [round(float(x), 4) for x in v]
        envs[k].close()

if mode in ("scene", "all"):
    # the arena's 24 agents scaled to the 16 (8 red + 8 blue) of the rung-3 rules
    arena1 = MapGenSpec(25, 25, {"wall": 10}, {"red": 8, "blue": 8}, num_agents=16, border_width=6, instance_border_width=0)
    arena4 = MapGenSpec(25, 25, {"wall": 10}, {"red": 2, "blue": 2}, num_agents=16, border_width=6, instance_border_width=0)
    recipes, shapes = {}, {}
    for name, scene in (("arena1", arena1), ("arena4", arena4)):
        H, W = shapes[name + "_scene"] = shapes[name + "_random"] = scene.map_height, scene.map_width
        n_walls = 10 * scene.instances_count
        recipes[name + "_scene"] = scene
        recipes[name + "_random"] = RandomMapSpec(H, W, {"wall": n_walls}, {"red": 8, "blue": 8}, border_width=6)   # the yardstick
    progs = {name: compile_spec(spec3, *shapes[name], max_objects=2048) for name in recipes}   # (1 344 border walls at 62 x 62)
    order = [(name, n) for name in recipes for n in (E, 64)]
    engs = {}
    for name, rec in recipes.items():
        engs[name] = BatchedMettaGrid(progs[name], generated_class_maps(rec, progs[name], [0]), [0], buffers="device", specialize=False)
        engs[name].set_map_generator(rec, [0])
    bufs = {(name, n): torch.zeros((n,) + shapes[name], dtype=torch.int16, device="cuda") for name, n in order}
    seeds = {E: (np.arange(E, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32), 64: np.arange(64, dtype=np.uint32) + 12345}
    ms = {k: [] for k in order}
    for r in range(rounds + 1):   # (round 0 warms up)
        for name, n in order:
            eng = engs[name]
            st = eng._ext_stream()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            eng.generate_maps(seeds[n], out=bufs[(name, n)])
            t1.record(st)
            t1.synchronize()
            if r:
                ms[(name, n)].append(t0.elapsed_time(t1))
    for (name, n), v in ms.items():
        out[f"generate_{name}_{n}_ms"] = stats(v, n)
    for name in ("arena1", "arena4"):
        for n in (E, 64):
            out[f"ratio_{name}_{n}"] = round(out[f"generate_{name}_scene_{n}_ms"]["median"] / out[f"generate_{name}_random_{n}_ms"]["median"], 3)
    for eng in engs.values():
        eng.close()
    del bufs
    prog = progs["arena4_scene"]
    pool = generated_class_maps(arena4, prog, range(16))
    EW = min(E, 16384)   # (2 048 object slots per env: a quarter of the batch keeps two engines of this size side by side small)
    out["wrapper_arena4_envs"] = EW
    envs = {"map_pool": MettaGridBatchedEnv(prog, EW, map_pool=pool, desync=True, episode_stats=False, specialize=False),
            "map_gen": MettaGridBatchedEnv(prog, EW, map_gen=arena4, desync=True, episode_stats=False, specialize=False)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for env in envs.values():
        env.reset()
    acts = [torch.randint(0, envs["map_gen"].transport_action_n, (EW * prog.num_agents,), generator=g, device="cuda", dtype=torch.int32) for _ in range(8)]
    wms = {k: [] for k in envs}
    for r in range(rounds + 1):
        for k, env in envs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for t in range(steps):
                env.step(acts[t % 8])
            t1.record()
            t1.synchronize()
            if r:
                wms[k].append(t0.elapsed_time(t1) / steps)
    for k, v in wms.items():
        out[f"wrapper_arena4_{k}_ms_per_step"] = stats(v)
        out[f"wrapper_arena4_{k}_ms_rounds"] = [round(float(x), 4) for x in v]
        envs[k].close()

if mode == "maze":
    rooms = {1: dict(agents={"red": 8, "blue": 8}), 4: dict(agents={"red": 2, "blue": 2})}
    common = dict(num_agents=16, border_width=6, instance_border_width=0)
    recipes = {}
    for n, kw in rooms.items():
        recipes[f"scene{n}"] = MapGenSpec(25, 25, {"wall": 10}, **kw, **common)   # the yardstick
        for alg in ("kruskal", "dfs"):
            recipes[f"maze{n}_{alg}"] = MazeGenSpec(25, 25, {"wall": 10}, **kw, **common, algorithm=alg)
    shapes = {name: (rec.map_height, rec.map_width) for name, rec in recipes.items()}
    progs = {name: compile_spec(spec3, *shapes[name], max_objects=4096) for name in recipes}   # (1 344 border + 4 x 298 maze walls)
    order = [(name, n) for name in recipes for n in (E, 64)]
    engs = {}
    for name, rec in recipes.items():
        engs[name] = BatchedMettaGrid(progs[name], generated_class_maps(rec, progs[name], [0]), [0], buffers="device", specialize=False)
        engs[name].set_map_generator(rec, [0])
    bufs = {(name, n): torch.zeros((n,) + shapes[name], dtype=torch.int16, device="cuda") for name, n in order}
    seeds = {E: (np.arange(E, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32), 64: np.arange(64, dtype=np.uint32) + 12345}
    ms = {k: [] for k in order}
    for r in range(rounds + 1):   # (round 0 warms up)
        for name, n in order:
            eng = engs[name]
            st = eng._ext_stream()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            eng.generate_maps(seeds[n], out=bufs[(name, n)])
            t1.record(st)
            t1.synchronize()
            if r:
                ms[(name, n)].append(t0.elapsed_time(t1))
    for (name, n), v in ms.items():
        out[f"generate_{name}_{n}_ms"] = stats(v, n)
    for name in recipes:
        if name.startswith("maze"):
            for n in (E, 64):
                yard = "scene" + name[4]
                out[f"ratio_{name}_{n}"] = round(out[f"generate_{name}_{n}_ms"]["median"] / out[f"generate_{yard}_{n}_ms"]["median"], 3)
    for eng in engs.values():
        eng.close()
    del bufs
    maze4, prog = recipes["maze4_kruskal"], progs["maze4_kruskal"]
    pool = generated_class_maps(maze4, prog, range(16))
    EW = min(E, 8192)   # (4 096 object slots per env)
    out["wrapper_maze4_envs"] = EW
    envs = {"map_pool": MettaGridBatchedEnv(prog, EW, map_pool=pool, desync=True, episode_stats=False, specialize=False),
            "map_gen": MettaGridBatchedEnv(prog, EW, map_gen=maze4, desync=True, episode_stats=False, specialize=False)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for env in envs.values():
        env.reset()
    acts = [torch.randint(0, envs["map_gen"].transport_action_n, (EW * prog.num_agents,), generator=g, device="cuda", dtype=torch.int32) for _ in range(8)]
    wms = {k: [] for k in envs}
    for r in range(rounds + 1):
        for k, env in envs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for t in range(steps):
                env.step(acts[t % 8])
            t1.record()
            t1.synchronize()
            if r:
                wms[k].append(t0.elapsed_time(t1) / steps)
    for k, v in wms.items():
        out[f"wrapper_maze4_{k}_ms_per_step"] = stats(v)
        out[f"wrapper_maze4_{k}_ms_rounds"] = [round(float(x), 4) for x in v]
        envs[k].close()
print(json.dumps(out), flush=True)
