"""The lane-per-agent area-effect kernel (mgx_aoe_kernel) on the cases of tests/aoe_cases.py, against the oracle.

E = 70: not a multiple of the kernel's four envs per workgroup (env 69 sits in the partial last one); env i has map seed i,
so the compared envs see every source count of a case's seed pattern (tests/test_aoe_cases_host.py test_source_counts, and
the witnesses that every case reaches what it is for in exactly these envs).  Every comparison is bit-exact: every
caller-visible buffer after every step, then the signature payloads and the error bits of all 70 envs (helpers.run_parity).
The same under each switch that moves this phase to other code, after the path bit is seen to flip.
"""
import numpy as np
import pytest

import aoe_cases as ac
import helpers as hp
from test_gpu_paths import CHECK_ENVS, default_paths

pytestmark = pytest.mark.gpu

E = 70
CASES = list(ac.AOE_SCENARIOS)
# the bits of this phase a case is meant to set by default, beside 'aoe_local' (which every case sets)
MEANT = {
    "aoe_words": ("aoe_prog_lds",),
    "aoe_chunks": ("aoe_prog_lds",),
    "aoe_chunks_wide": ("aoe_prog_lds", "tick_in_aoe", "cov_in_aoe"),
    "aoe_ops": ("tick_in_aoe", "cov_in_aoe"),
    "aoe_stats": ("tick_in_aoe", "cov_in_aoe"),
}
# switch -> (the bit it clears, the cases it applies to: those whose default sets the bit)
SWITCHES = {
    "MGX_AOE_SERIAL": ("aoe_local", CASES),
    "MGX_AOE_PROG_HBM": ("aoe_prog_lds", [n for n in CASES if "aoe_prog_lds" in MEANT[n]]),
    "MGX_TICK_SERIAL": ("tick_in_aoe", [n for n in CASES if "tick_in_aoe" in MEANT[n]]),
}
# agent stats the kernel stages per lane (MGX_VERBOSE reports the count): the two cases past MGX_AOE_MAX_STATS = 32
STAGED_ALL = ("aoe_ops", "aoe_stats")


@pytest.mark.parametrize("name", CASES)
def test_parity(name, monkeypatch, capfd):
    monkeypatch.setenv("MGX_VERBOSE", "1")
    paths = default_paths(name)
    report = capfd.readouterr().err
    monkeypatch.delenv("MGX_VERBOSE")
    assert paths["aoe_local"], f"{name}: mgx_aoe_is_target_local refuses the program"
    for bit in MEANT[name]:
        assert paths[bit], f"{name}: '{bit}' is not set"
    if name in STAGED_ALL:
        assert "aoe kernel: 32 agent stats staged per lane" in report, report
    hp.run_parity(name, E, CHECK_ENVS)


@pytest.mark.parametrize("switch,name", [(s, n) for s, (_, names) in SWITCHES.items() for n in names])
def test_parity_under_switch(switch, name, monkeypatch):
    bit = SWITCHES[switch][0]
    assert default_paths(name)[bit], f"{name}: the default does not take the '{bit}' side"
    monkeypatch.setenv(switch, "1")
    assert not default_paths(name)[bit], f"{name}: {switch}=1 did not clear '{bit}'"
    hp.run_parity(name, E, CHECK_ENVS)


def test_chunks_wide_equals_its_serial_twin_in_every_env(monkeypatch):
    """Two engines of `aoe_chunks_wide` on the same maps, seeds and actions — the kernel, and the extended world kernel's own
    area-effect phase (MGX_AOE_SERIAL=1) — agree in ALL 70 envs: every caller-visible buffer after every step, every
    object and every stat at the end."""
    from mettagrid_amd.engine import BatchedMettaGrid
    name = "aoe_chunks_wide"
    spec_f, map_f, steps, invalid = hp.scenario(name)
    maps = [map_f(s) for s in range(E)]
    prog = hp.compile_scenario(name, spec_f(), *maps[0].shape)
    cms = np.stack([prog.class_map(m) for m in maps])
    seeds = np.arange(E, dtype=np.uint32) * 7 + 3
    acts = [hp.make_actions(prog, i, steps, invalid) for i in range(E)]
    fast = BatchedMettaGrid(prog, cms, seeds, buffers="host")
    serial = None
    try:
        monkeypatch.setenv("MGX_AOE_SERIAL", "1")
        serial = BatchedMettaGrid(prog, cms, seeds, buffers="host")
        monkeypatch.delenv("MGX_AOE_SERIAL")
        assert fast.paths["aoe_local"] and not serial.paths["aoe_local"]
        for t in range(steps):
            for eng in (fast, serial):
                eng.actions[:] = np.concatenate([acts[i][0][t] for i in range(E)])
                eng.vibe_actions[:] = np.concatenate([acts[i][1][t] for i in range(E)])
                eng.step()
            a, b = fast.snapshot(), serial.snapshot()
            for k in hp.SNAPSHOT_KEYS:
                if not np.array_equal(a[k], b[k]):
                    rows = np.nonzero((np.asarray(a[k]) != np.asarray(b[k])).reshape(E * prog.num_agents, -1).any(axis=1))[0]
                    raise AssertionError(f"step {t + 1}: '{k}' differs in rows {rows[:8].tolist()} (env = row // {prog.num_agents})")
        assert fast.poll_errors()[0] == 0 and serial.poll_errors()[0] == 0
        for i in range(E):
            assert np.array_equal(fast.raw_objects(i), serial.raw_objects(i)), f"objects of env {i} differ"
            for p, q in zip(fast.raw_stats(i), serial.raw_stats(i)):
                assert np.array_equal(p, q), f"stats of env {i} differ"
    finally:
        fast.close()
        if serial is not None:
            serial.close()
