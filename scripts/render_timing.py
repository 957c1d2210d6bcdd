"""Cost of rendering (mgx_render_rgb / mgx_render_cells) at the rung-3 headline shape (65 536 envs, 32x32
maps, 16 agents), in one process; the variants alternate round by round (interleave what you compare, report the spread) and
per variant the median over the rounds is reported with min / max and the coefficient of variation:
  (i)   rgb_64 / rgb_1024     render_rgb of 64 / 1 024 envs at s = 8 (256x256x3 bytes per frame), `reps` back-to-back launches
                              between two events on the engine's stream
        copy_64 / copy_1024   the yardstick: a device-to-device copy of the same number of bytes, timed the same way;
                              `ratio` = rgb / copy
  (ii)  step_off / step_64 / step_1024   wall time per MettaGridBatchedEnv.step (device restarts from a pool, random actions
                              made up front) with render_envs off, 64 envs and 1 024 envs, `steps` steps per round, the
                              device drained at the end of the round
  (iii) ansi_one              wall time of render_cells([env]) + render.ansi for one env
Prints one JSON line.
Usage (GPU box): python scripts/render_timing.py [envs] [rounds] [reps] [steps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets, render  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.envs import MettaGridBatchedEnv  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
S = 8


def stats(a) -> dict:
    a = np.asarray(a, dtype=np.float64)
    return {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4),
            "cv_pct": round(float(a.std() / a.mean() * 100), 2)}


def main() -> None:
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    pool = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(16))
    watch = {0: None, 64: np.arange(64) * (E // 64), 1024: np.arange(1024) * (E // 1024)}
    envs = {n: MettaGridBatchedEnv(prog, E, map_pool=pool, seed=1, specialize=False, episode_stats=False, render_envs=w, render_scale=S)
            for n, w in watch.items()}
    for env in envs.values():
        env.reset()
    dev = envs[0].engine.obs.device
    gen = torch.Generator(device=dev).manual_seed(1)
    acts = [torch.randint(0, envs[0].transport_action_n, (envs[0].num_agents,), dtype=torch.int32, device=dev, generator=gen) for _ in range(8)]
    for env in envs.values():   # warm-up: every kernel of every variant has run
        for a in acts:
            env.step(a)
    torch.cuda.synchronize()

    # ---- (i) the kernel against a copy of the same bytes, on the engine's stream ----
    eng = envs[0].engine
    eng.set_render_tiles(scale=S)
    stream = eng._ext_stream()
    frame_bytes = 32 * S * 32 * S * 3
    bufs = {n: (torch.empty(n * frame_bytes, dtype=torch.uint8, device=dev), torch.empty(n * frame_bytes, dtype=torch.uint8, device=dev))
            for n in (64, 1024)}
    torch.cuda.synchronize()

    def copy(n):
        with torch.cuda.stream(stream):
            bufs[n][1].copy_(bufs[n][0])

    kernel_variants = {}
    for n in (64, 1024):
        kernel_variants[f"rgb_{n}"] = (lambda n=n: eng.render_rgb(watch[n], bufs[n][0]))
        kernel_variants[f"copy_{n}"] = (lambda n=n: copy(n))

    def timed(f) -> float:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(reps):
            f()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    for f in kernel_variants.values():
        f()
    eng.sync()
    ms = {k: [] for k in kernel_variants}
    for _ in range(rounds):
        for name, f in kernel_variants.items():
            ms[name].append(timed(f))
    out = {"envs": E, "scale": S, "rounds": rounds, "reps": reps, "steps_per_round": steps, "lib": os.path.basename(eng.L._name)}
    for name in kernel_variants:
        n = int(name.split("_")[1])
        out[name] = dict(stats(ms[name]), unit="ms", bytes=n * frame_bytes)
        out[name]["GBps"] = round(n * frame_bytes / (out[name]["median"] * 1e-3) / 1e9, 1)
    for n in (64, 1024):
        out[f"ratio_{n}"] = round(out[f"rgb_{n}"]["median"] / out[f"copy_{n}"]["median"], 3)
    # the frames the timed launches wrote are the ones the rule asks for
    want = render.rgb_host(eng.render_cells(watch[64][:4]), *eng.render_tiles)
    assert np.array_equal(bufs[64][0][:4 * frame_bytes].cpu().numpy().reshape(want.shape), want)

    # ---- (ii) the wrapper step ----
    step_ms = {n: [] for n in envs}
    for _ in range(rounds):
        for n, env in envs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                env.step(acts[k % len(acts)])
            torch.cuda.synchronize()
            step_ms[n].append((time.perf_counter() - t0) * 1e3 / steps)
    for n in envs:
        out["step_off" if n == 0 else f"step_{n}"] = dict(stats(step_ms[n]), unit="ms per step")

    # ---- (iii) one env as text ----
    names = render.class_type_names(prog)
    ansi_ms = []
    for r in range(max(rounds, 5) * 4):
        t0 = time.perf_counter()
        text = render.ansi(eng.render_cells([r % E])[0], names)
        ansi_ms.append((time.perf_counter() - t0) * 1e3)
    assert text.count("\n") == 31
    out["ansi_one"] = dict(stats(ansi_ms), unit="ms")
    for env in envs.values():
        env.close()
    print(json.dumps(out), flush=True)


main()
