"""The oracle restatement against the REAL reference engine: tests/golden/vs_reference/traces.npz holds what the reference
(oracle/_ref/mettagrid_c*.so, built from the reference sources by `make -C oracle ref`) produced for these cases, written
by tests/golden/make_vs_reference.py — per step a digest of every caller-visible buffer, the final signature payload."""
import json
import os

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
from mettagrid_amd import signature as sg
from mettagrid_amd.compiler import compile_spec

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "vs_reference", "traces.npz"))

def _json(key: str):
    return json.loads(bytes(GOLD[key]).decode())


@pytest.mark.parametrize("name", list(hp.SCENARIOS))
@pytest.mark.parametrize("seed", [5, 6])
def test_oracle_equals_reference(name, seed):
    spec_f, map_f, steps, invalid = hp.SCENARIOS[name]
    spec, cells = spec_f(), map_f(seed)
    prog = hp.compile_scenario(name, spec, *cells.shape)
    want = GOLD[f"{name}_s{seed}/digests"]
    assert want.shape == (steps + 1, len(hp.SNAPSHOT_KEYS))
    ora = op.OracleSim(prog, prog.class_map(cells), seed)
    acts, vibes = hp.make_actions(prog, seed, steps, invalid)

    def check(t):
        got = hp.snapshot_digests(ora.snapshot())
        bad = [k for k, a, b in zip(hp.SNAPSHOT_KEYS, got, want[t]) if a != b]
        assert not bad, f"{name} seed {seed} step {t}: {bad} differ from the reference"

    check(0)
    for t in range(steps):
        ora.step(acts[t], vibes[t])
        check(t + 1)
    pa = _json(f"{name}_s{seed}/payload")
    pb = json.loads(json.dumps(hp.payload_from_raw(prog, ora.raw_objects(), ora.current_stat_reward(), ora.raw_stats(),
                                                   ora.snapshot(), ora.current_step, seed)))
    assert pa == pb, hp.diff_payload(pa, pb)


def test_restated_rng_equals_libstdcxx():
    L = op.lib()
    for seed in (0, 1, 42, 123456789):
        for n in (1, 2, 3, 4, 5, 16, 24, 63, 64, 255):
            assert L.mgxo_selftest_shuffle(seed, n, 300) == 0


def test_reference_inventory_token_order_follows_emulated_unordered_map():
    """Observation token order of inventory items is libstdc++ unordered_map order; the spec's dict
    order of initial inventories must survive compile -> oracle exactly as it does config -> reference."""
    for i, initial in enumerate(hp.INVENTORY_ORDER):
        spec, cells = hp.inventory_order_case(initial)
        prog = compile_spec(spec, *cells.shape)
        ora = op.OracleSim(prog, prog.class_map(cells), 1)
        assert np.array_equal(GOLD[f"inventory_order/{i}/obs"], ora.snapshot()["obs"]), initial


def test_far_invalid_action_indices_match_reference_stat_keys():
    """The reference keys "action.invalid_index.<k>" by the raw index (mettagrid_c.cpp:916-918); the oracle's (k, count)
    pairs must produce the same stats dict."""
    spec, cells, prog, steps = hp.invalid_index_case()
    ora = op.OracleSim(prog, prog.class_map(cells), hp.INVALID_INDEX_SEED)
    for acts, vibes in steps:
        ora.step(acts, vibes)
    assert ora.error == 0
    mine = sg.stats_dicts(prog, *ora.raw_stats(), extra=ora.invalid_index_extra())
    theirs = _json("invalid_index")
    assert len(theirs) == prog.num_agents
    for i in range(prog.num_agents):
        got = {k: v for k, v in mine["agent"][i].items() if k.startswith("action.invalid_index")}
        assert json.loads(json.dumps(got)) == theirs[i]
