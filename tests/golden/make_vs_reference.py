"""Generates tests/golden/vs_reference/traces.npz, the fixture of tests/test_oracle_vs_reference.py, from the REAL reference
engine (oracle/_ref, built by `make -C oracle ref` where the reference sources exist).

Run where oracle/_ref exists:  python tests/golden/make_vs_reference.py
Contents (data only; no reference source is copied):
  * ``<scenario>_s<seed>/digests``  uint32 [steps + 1, 6]: ``helpers.snapshot_digests`` of the reference's caller-visible
    buffers before the first step and after every step, for every scenario of tests/helpers.py and seeds 5 and 6
    (action traces: ``helpers.make_actions``);
  * ``<scenario>_s<seed>/payload``  the generalised signature payload (JSON bytes) after the last step;
  * ``inventory_order/<i>/obs``     the reference's observations at step 0 of the helpers.INVENTORY_ORDER cases;
  * ``invalid_index``               JSON bytes: the reference's per-agent "action.invalid_index.*" stats after the
    helpers.INVALID_INDEX_STEPS actions on rung 1.
"""
import json
import os
import platform
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import helpers as hp  # noqa: E402
from mettagrid_amd import signature as sg  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402

OUT = os.path.join(HERE, "vs_reference", "traces.npz")
SEEDS = (5, 6)


def main() -> None:
    import ref_driver as rd
    if not rd.ref_available():
        raise SystemExit("oracle/_ref is not built: run `make -C oracle ref` where the reference sources exist")
    out = {}
    for name, (spec_f, map_f, steps, invalid) in hp.SCENARIOS.items():
        for seed in SEEDS:
            spec, cells = spec_f(), map_f(seed)
            prog = hp.compile_scenario(name, spec, *cells.shape)
            ref = rd.RefSim(spec, cells, seed, prog)
            acts, vibes = hp.make_actions(prog, seed, steps, invalid)
            dig = [hp.snapshot_digests(ref.snapshot())]
            for t in range(steps):
                ref.step(acts[t], vibes[t])
                dig.append(hp.snapshot_digests(ref.snapshot()))
            c = ref.c
            payload = sg.payload(c.grid_objects(), c.get_episode_stats(), c.action_success(), c.get_episode_rewards(),
                                 c.current_step, seed)
            out[f"{name}_s{seed}/digests"] = np.stack(dig)
            out[f"{name}_s{seed}/payload"] = np.frombuffer(json.dumps(payload).encode(), dtype=np.uint8)
    for i, initial in enumerate(hp.INVENTORY_ORDER):
        spec, cells = hp.inventory_order_case(initial)
        prog = compile_spec(spec, *cells.shape)
        out[f"inventory_order/{i}/obs"] = rd.RefSim(spec, cells, 1, prog).snapshot()["obs"]
    spec, cells, prog, steps = hp.invalid_index_case()
    ref = rd.RefSim(spec, cells, hp.INVALID_INDEX_SEED, prog)
    for acts, vibes in steps:
        ref.step(acts, vibes)
    stats = [{k: v for k, v in a.items() if k.startswith("action.invalid_index")} for a in ref.c.get_episode_stats()["agent"]]
    out["invalid_index"] = np.frombuffer(json.dumps(stats).encode(), dtype=np.uint8)
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    meta = {"seeds": list(SEEDS), "toolchain": gxx, "python": platform.python_version()}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
