"""Generates tests/golden/vs_reference/aoe_traces.npz, the fixture of tests/test_aoe_cases_host.py, from the REAL reference
engine (oracle/_ref, built by `make -C oracle ref` where the reference sources exist): what make_vs_reference.py writes for
helpers.SCENARIOS, for the cases of tests/aoe_cases.py.

Run where oracle/_ref exists:  python tests/golden/make_aoe_vs_reference.py
Contents (data only; no reference source is copied):
  * ``<case>_s<seed>/digests``  uint32 [steps + 1, 6]: ``helpers.snapshot_digests`` of the reference's caller-visible buffers
    before the first step and after every step, for every case of aoe_cases.AOE_SCENARIOS and seeds 5 and 6 (action traces:
    ``helpers.make_actions``);
  * ``<case>_s<seed>/payload``  the generalised signature payload (JSON bytes) after the last step.
A spec the reference refuses (a config error) is not a legal game: the case has to change, not this script.
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

import aoe_cases as ac  # noqa: E402
import helpers as hp  # noqa: E402
from mettagrid_amd import signature as sg  # noqa: E402

OUT = os.path.join(HERE, "vs_reference", "aoe_traces.npz")
SEEDS = (5, 6)


def main() -> None:
    import ref_driver as rd
    if not rd.ref_available():
        raise SystemExit("oracle/_ref is not built: run `make -C oracle ref` where the reference sources exist")
    out = {}
    for name, (spec_f, map_f, steps, invalid) in ac.AOE_SCENARIOS.items():
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
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    meta = {"seeds": list(SEEDS), "toolchain": gxx, "python": platform.python_version()}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
