"""Every code path mgx_create chooses (mgx_create_paths / BatchedMettaGrid.paths), on both sides, against the oracle.

1. Coverage table: the paths every scenario of helpers.SCENARIOS, helpers.LIMIT_SCENARIOS and aoe_cases.AOE_SCENARIOS
   takes by default are pinned (EXPECTED), and every bit is seen set and clear across the table — a refactor that moves a scenario off a path, or a
   new path no scenario reaches, fails here.  Bits only an environment switch can flip are listed in FORCED_ONLY.
2. Forced fallbacks: each switch of mgx_create, on scenarios whose default takes the fast side; the bit must flip, then
   the run is compared with the oracle after every step (E = 70: envs across the 32-env wavefront and the 64-env
   workgroup boundaries) and by signature payload at the end.
"""
import pytest

import helpers as hp
from aoe_cases import AOE_SCENARIOS
from mettagrid_amd.engine import PATH_BITS

pytestmark = pytest.mark.gpu

# bits no scenario's default clears or sets: the switch that flips them, and why
FORCED_ONLY = {}

# set bits of each scenario's default paths (E = 1, map seed 0)
EXPECTED = {
    'rung1': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'rung1_invalid': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'rung2': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'rung3': ['duo', 'gen', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'rung3_flat_damage': ['duo', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'torture': ['prog_lds', 'shadow', 'tick_split'],
    'torture_terminal': ['prog_lds', 'shadow', 'tick_split'],
    'rung4': ['X', 'aoe_local', 'aoe_prog_lds', 'prog_lds', 'rewards_ext'],
    'rung4_full': ['X', 'act_map', 'act_par', 'aoe_local', 'aoe_prog_lds', 'cov_in_aoe', 'flat_top', 'gen', 'obs_512', 'prog_lds', 'rewards_mid', 'shadow', 'tick_in_aoe'],
    'rung4_truncating': ['X', 'aoe_local', 'aoe_prog_lds', 'prog_lds', 'rewards_ext'],
    'dynamic': ['X', 'prog_lds', 'rewards_mid', 'x_aoe_lds'],
    'wide': ['duo', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'crowd': ['duo', 'rewards_early', 'shadow', 'tick_split', 'world_lds_64k'],
    'torture_base10': ['prog_lds', 'shadow', 'tick_split'],
    'keyhole': ['duo', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'letterbox': ['duo', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'minmax': ['duo', 'prog_lds', 'shadow', 'tick_split'],
    'thirteen': ['prog_lds', 'shadow', 'tick_split'],
    'lit': ['X', 'act_map', 'act_par', 'flat_top', 'prog_lds', 'rewards_ext', 'shadow', 'x_aoe_lds'],
    'delta': ['X', 'act_map', 'act_par', 'flat_top', 'prog_lds', 'rewards_mid', 'shadow', 'x_aoe_lds'],
    'agents_lean_max': ['duo', 'rewards_early', 'shadow', 'tick_split', 'world_lds_64k'],
    'agents_ext_max': ['X', 'aoe_local', 'aoe_prog_lds', 'cov_in_aoe', 'flat_top', 'obs_512', 'rewards_mid', 'tick_in_aoe', 'world_lds_64k'],
    'map_max_default': ['duo', 'gen', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'map_max_few': ['duo', 'gen', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'window15': ['duo', 'prog_lds', 'rewards_early', 'shadow', 'tick_split'],
    'ceiling_b2': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'ceiling_b10': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'ceiling_b256': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'tags': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'nest4_lean': ['duo', 'prog_lds', 'rewards_early', 'shadow'],
    'nest4_x': ['X', 'act_map', 'act_par', 'flat_top', 'prog_lds', 'rewards_mid', 'shadow', 'x_aoe_lds'],
    'nest6_x': ['X', 'prog_lds', 'rewards_mid', 'x_aoe_lds'],
    'query3': ['X', 'act_map', 'act_par', 'flat_top', 'prog_lds', 'rewards_ext', 'shadow', 'x_aoe_lds'],
    'aoe_words': ['X', 'aoe_local', 'aoe_prog_lds', 'prog_lds', 'rewards_ext'],
    'aoe_chunks': ['X', 'aoe_local', 'aoe_prog_lds', 'prog_lds', 'rewards_ext'],
    'aoe_chunks_wide': ['X', 'aoe_local', 'aoe_prog_lds', 'cov_in_aoe', 'flat_top', 'obs_512', 'prog_lds', 'rewards_mid', 'tick_in_aoe'],
    'aoe_ops': ['X', 'aoe_local', 'cov_in_aoe', 'prog_lds', 'rewards_ext', 'tick_in_aoe'],
    'aoe_stats': ['X', 'aoe_local', 'cov_in_aoe', 'prog_lds', 'rewards_ext', 'tick_in_aoe'],
}

# switch -> (value, the bit it clears, scenarios whose default has that bit set)
FALLBACKS = {
    "MGX_PROG_LDS": ("0", "prog_lds", ["torture", "lit", "rung4", "dynamic"]),
    "MGX_AOE_SERIAL": ("1", "aoe_local", ["rung4", "rung4_full", "rung4_truncating"]),
    "MGX_TICK_SERIAL": ("1", "cov_in_aoe", ["rung4_full"]),
    "MGX_AOE_PROG_HBM": ("1", "aoe_prog_lds", ["rung4", "rung4_full"]),
    "MGX_NO_FLAT_TOP": ("1", "flat_top", ["rung4_full", "lit", "delta"]),
    "MGX_NO_TICK_SPLIT": ("1", "tick_split", ["torture", "rung3"]),
    "MGX_REWARDS_LATE": ("1", "rewards_mid", ["rung4_full", "dynamic", "delta"]),
    "MGX_OBS_256": ("1", "obs_512", ["rung4_full", "agents_ext_max"]),
}
CHECK_ENVS = (0, 31, 32, 63, 64, 69)


def default_paths(name: str) -> dict:
    eng = hp.create_one(name)
    try:
        return eng.paths
    finally:
        eng.close()


def test_coverage_table():
    names = list(hp.SCENARIOS) + list(hp.LIMIT_SCENARIOS) + list(AOE_SCENARIOS)
    table = {n: default_paths(n) for n in names}
    got = {n: sorted(b for b, on in p.items() if on) for n, p in table.items()}
    listing = "\n".join(f"    {n!r}: {got[n]}," for n in names)
    assert got == EXPECTED, f"default paths differ from EXPECTED; the table now reads:\n{listing}"
    for bit in PATH_BITS:
        sides = {table[n][bit] for n in names}
        if bit in FORCED_ONLY:
            assert len(sides) == 1, f"'{bit}' is listed in FORCED_ONLY but scenarios now take both sides"
        else:
            assert sides == {True, False}, f"no scenario takes the {'set' if False in sides else 'clear'} side of '{bit}'"


def test_every_switch_names_a_bit():
    for bit in [b for _, b, _ in FALLBACKS.values()] + list(FORCED_ONLY):
        assert bit in PATH_BITS, bit


@pytest.mark.parametrize("switch", list(FALLBACKS))
def test_forced_fallback_parity(switch, monkeypatch):
    value, bit, names = FALLBACKS[switch]
    for name in names:
        assert default_paths(name)[bit], f"{name}: the default no longer takes the '{bit}' side; pick another scenario"
    monkeypatch.setenv(switch, value)
    for name in names:
        forced = default_paths(name)
        assert not forced[bit], f"{name}: {switch}={value} did not clear '{bit}'"
        hp.run_parity(name, 70, CHECK_ENVS)
