"""Per-phase shader-clock breakdown of the world kernel (needs a -DMGX_WORLD_TIMING build, see MGX_LIB).
Usage: MGX_LIB=mettagrid_amd/libmgx_timing.so python scripts/world_timing.py [steps]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import engine, presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
E, A = 65536, prog.num_agents
cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
eng = engine.BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), device=0, buffers="device")
lib = engine.load_lib()
n = len(prog.action_names)
gen = torch.Generator(device="cuda").manual_seed(42)
pa = torch.randint(0, n, (8, E * A), dtype=torch.int32, device="cuda", generator=gen)
pv = torch.randint(0, n, (8, E * A), dtype=torch.int32, device="cuda", generator=gen)
ext = torch.cuda.ExternalStream(eng.stream)
out = (C.c_ulonglong * 16)()
out2 = (C.c_ulonglong * 16)()
for t in range(5 + steps):
    if t == 5:
        eng.sync()
        lib.mgx_debug_world_cycles(out, 1)
        lib.mgx_debug_world_run_cycles((C.c_ulonglong * 16)(), 1)
        lib.mgx_debug_obs_cycles(out2, 1)
    with torch.cuda.stream(ext):
        eng.actions.copy_(pa[t % 8]); eng.vibe_actions.copy_(pv[t % 8])
        eng.step()
eng.sync()
lib.mgx_debug_world_cycles(out, 0)
names = ["stage agents", "shuffle", "stream0 (move/noop)", "stream1 (vibe)", "on_tick", "coverage", "  do_move (in streams)", "  action bookkeeping",
         "resolve move targets"]
waves = (E + 63) // 64
print(f"move_fast {eng.move_fast}  world_variant {eng.world_variant}")
for k, nm in enumerate(names):
    print(f"{nm:28s} {out[k] / steps / waves:12.0f} cycles / wave / step")
# event counts of the primary stream (MGX_COUNT), first wavefront of every workgroup (32 envs) like the cycle totals
print(f"{'stream0 trips':28s} {out[9] / steps / waves:12.2f} / wave / step")
print(f"{'run-ahead actions':28s} {out[10] / steps / waves / 32:12.2f} / env / step   (of {A} agents)")
print(f"{'general-path dispatches':28s} {out[11] / steps / waves / 32:12.2f} / env / step")
print(f"{'  of them stale entries':28s} {out[12] / steps / waves / 32:12.3f} / env / step")
# the primary stream split (mgx_dbg_run): the run-ahead loop, the fence behind it, the general-path trips, the rest
run = (C.c_ulonglong * 16)()
lib.mgx_debug_world_run_cycles(run, 0)
a, b, c = (run[k] / steps / waves for k in range(3))
s0 = out[2] / steps / waves
for nm, v in [("(a) run-ahead loop", a), ("(b) fence + barrier behind it", b), ("(c) footprints + dispatch_one", c), ("(d) rest", s0 - a - b - c)]:
    print(f"  {nm:26s} {v:12.0f} cycles / wave / step   {100 * v / max(s0, 1):5.1f} % of stream0")
# (c) per general-path trip: up to the call, up to the first lane's entry of apply_top, to the last lane's return, the rest + the fence
for k, nm in [(4, "(c1) footprints + pairing"), (5, "(c2) dispatch, to apply_top"), (6, "(c3) inside apply_top"), (7, "(c4) rest + pair's fence")]:
    v = run[k] / steps / waves
    print(f"    {nm:28s} {v:10.0f} cycles / wave / step   {100 * v / max(c, 1):5.1f} % of (c)")
print(f"{'run-ahead loop iterations':28s} {run[3] / steps / waves:12.2f} / wave / step   (maximum over the lanes, summed over the trips)")
print(f"{'trips that enter apply_top':28s} {run[13] / steps / waves:12.2f} / wave / step")
# calls inside stream 0's dispatches, each the start of a round trip: per general-path dispatch (and per env and step)
# (memory-path calls only: an instance with dispatch records answers these from registers for the dispatch's two objects)
disp = max(out[11], 1)
for k, nm in [(8, "inv_row"), (9, "cls_of"), (10, "agent_of"), (11, "inv() reads"), (12, "on_inventory_change")]:
    print(f"  {nm + ' calls':26s} {run[k] / disp:12.2f} / general-path dispatch   {run[k] / steps / waves / 32:8.3f} / env / step")
lib.mgx_debug_obs_cycles(out2, 0)
print("observation kernel, thread 0 of every workgroup:")
for k, nm in [(8, "stage grid/agents"), (9, "object token cache"), (10, "first observer"), (11, "encode 4 agents"),
              (12, "barrier wait"), (13, "visited + token stats"), (14, "rewards")]:
    print(f"{nm:28s} {out2[k] / steps / E:12.0f} cycles / workgroup / step")
