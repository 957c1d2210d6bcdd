"""GPU: a kernel's dynamic-LDS limit is shared by every engine of the process and only ever raised (csrc/mgx_host.h
MgxLdsLimit).  Each case creates an engine that needs much LDS in a kernel unit, then one that needs little in the same
unit on the same device, and steps them alternately, both compared with the oracle after every step: the second
mgx_create must not lower the limit under the first engine.  Pairs from the path table of test_gpu_paths.py."""
import pytest

import helpers as hp

pytestmark = pytest.mark.gpu

E, STEPS, CHECK_ENVS = 2, 12, (0, 1)
# The lean world unit exists once per constant-memory slot and engines take the slots round-robin: with as many small
# engines as there are slots, one of them shares the big engine's slot (and its kernels' limit) whichever that is.
LEAN_SLOTS = 2

PAIRS = {
    # unit(s): (the engine that needs much, the one that needs little, how many of those)
    "lean_world": ("crowd", "keyhole", LEAN_SLOTS),            # world_lds_64k; two programs through one constant-memory slot
    "ext_world_aoe_obs512": ("agents_ext_max", "rung4", 1),    # world_lds_64k, aoe_local, obs_512
    "ext_dispatch": ("rung4_full", "lit", 1),                  # act_par, aoe_prog_lds
}


@pytest.mark.parametrize("case", list(PAIRS))
def test_smaller_engine_does_not_lower_the_limit(case):
    big, small, n_small = PAIRS[case]
    runs = []
    try:
        runs.append(hp.ParityRun(big, E, CHECK_ENVS, STEPS))
        for _ in range(n_small):
            runs.append(hp.ParityRun(small, E, CHECK_ENVS, STEPS))
        for _ in range(STEPS):
            for run in runs:
                run.step()
        for run in runs:
            run.finish()
    finally:
        for run in runs:
            run.close()
