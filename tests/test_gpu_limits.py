"""Capacity limits: each accepted size at its maximum against the oracle, and the next size refused by mgx_create on the
host (MGX_ERR_PROGRAM, before any kernel runs).  The sizes are those of helpers.LIMIT_SCENARIOS, which DESIGN.md
"Known limits" states."""
import numpy as np
import pytest

import helpers as hp
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid, MgxError

pytestmark = pytest.mark.gpu

# envs across the 32-env wavefront (extended world kernel) and 64-env workgroup (lean world kernel) boundaries
E = 65
CHECK_ENVS = (0, 31, 32, 63, 64)


def refused(spec, grid, match: str, max_objects=None) -> None:
    prog = compile_spec(spec, *grid.shape, max_objects=max_objects)
    with pytest.raises(MgxError, match=r"error -3: .*" + match):
        BatchedMettaGrid(prog, prog.class_map(grid)[None], np.zeros(1, np.uint32), buffers="host")


def accepted(spec, grid, max_objects=None) -> dict:
    prog = compile_spec(spec, *grid.shape, max_objects=max_objects)
    eng = BatchedMettaGrid(prog, prog.class_map(grid)[None], np.zeros(1, np.uint32), buffers="host")
    try:
        return eng.paths
    finally:
        eng.close()


def test_most_agents_lean():
    n = hp.LEAN_MAX_AGENTS
    assert accepted(hp.lean_agents_spec(n), hp.lean_agents_map(0, n))["world_lds_64k"]
    refused(hp.lean_agents_spec(n + 1), hp.lean_agents_map(0, n + 1), r"149 agents per env are too many for the lean world kernel")
    hp.run_parity("agents_lean_max", E, CHECK_ENVS)


def test_most_agents_extended():
    """The extended kernel stages 32 envs per workgroup: its LDS holds MGX_MAX_AGENTS (254); 255 is refused by the
    compiler (test_limits_host.py)."""
    n = hp.EXT_MAX_AGENTS
    assert n == 254
    p = accepted(hp.ext_agents_spec(n), hp.ext_agents_map(0, n))
    assert p["X"] and p["world_lds_64k"]
    hp.run_parity("agents_ext_max", E, CHECK_ENVS)


def test_map_at_default_max_objects():
    n = hp.MAP_MAX_DEFAULT
    from mettagrid_amd import presets
    accepted(presets.rung3_spec(), hp.edge_map(n, n, 0))
    refused(presets.rung3_spec(), hp.edge_map(n + 1, n + 1, 0), "too large for the LDS staging of the observation kernel")
    hp.run_parity("map_max_default", E, CHECK_ENVS)


def test_map_with_few_objects():
    """The largest map with a small max_objects: rows and columns up to 254 in the 8-bit position fields."""
    h, w = hp.MAP_MAX_FEW
    from mettagrid_amd import presets
    accepted(presets.rung3_spec(), hp.edge_map(h, w, 0), hp.MAP_FEW_OBJECTS)
    hp.run_parity("map_max_few", E, CHECK_ENVS)


def test_window_15x15():
    env, step = hp.WINDOW15_FULL
    stats = hp.run_parity("window15", E, CHECK_ENVS + (env,))["game"]
    assert stats["tokens_written"] > 0 and stats["tokens_dropped"] == 0
    # the oracle's view of that env: at `step` an agent's row is full to the last slot
    import oracle_py as op
    spec_f, map_f, steps, invalid = hp.LIMIT_SCENARIOS["window15"]
    grid = map_f(env)
    prog = hp.compile_scenario("window15", spec_f(), *grid.shape)
    o = op.OracleSim(prog, prog.class_map(grid), env * 7 + 3)
    o.reinit_buffers()
    acts = hp.make_actions(prog, env, steps, invalid)
    for t in range(step):
        o.step(acts[0][t], acts[1][t])
    assert (o.snapshot()["obs"][:, :, 0] != 0xFF).sum(axis=1).max() == prog.num_tokens


@pytest.mark.parametrize("name", ["ceiling_b2", "ceiling_b10", "ceiling_b256"])
def test_inventory_at_the_uint16_ceiling(name):
    hp.run_parity(name, E, CHECK_ENVS)


def test_tags():
    hp.run_parity("tags", E, CHECK_ENVS)
    refused(hp.tags_spec(64), hp.tags_map(0), "more than 63 tags on one class")


def test_object_slots_within_the_vm_packing():
    """The handler VM holds slot ids as (id + 2) & 0xFFFF: 65534 slots are the most the compiler and mgx_create accept,
    and at 255x255 the observation kernel's LDS staging refuses that many anyway (DESIGN.md Known limits)."""
    from mettagrid_amd import presets
    refused(presets.rung3_spec(), hp.edge_map(255, 255, 0), "observation kernel", max_objects=65534)
    accepted(presets.rung3_spec(), hp.edge_map(255, 255, 0), hp.MAX_SLOTS_AT_255)
    refused(presets.rung3_spec(), hp.edge_map(255, 255, 0), "observation kernel", max_objects=hp.MAX_SLOTS_AT_255 + 1)


def test_handler_nesting_on_both_vms(monkeypatch):
    """Handler chains at each VM's last frame: 4 frames on the register VM (lean programs; extended programs whose chains
    fit it take it by default — flat_top) and 6 on the LDS VM (MGX_NO_FLAT_TOP, and by default for deeper chains).  An
    on_use tree runs above the move handler that reached it: 3 and 5 levels here.  No generated handler code exists for
    these programs (it is built for the presets' handler tables only), so all of them run the interpreter, with or
    without MGX_NO_GEN."""
    for name, flat in (("nest4_lean", False), ("nest4_x", True), ("nest6_x", False)):
        p = hp.create_one(name)
        paths = p.paths
        p.close()
        assert paths["flat_top"] == flat and not paths["gen"], (name, paths)
        hp.run_parity(name, E, CHECK_ENVS)
    # a fifth frame is refused for lean programs (the register VM is all they have) ...
    refused(hp.nesting_spec(4, extended=False), hp.nesting_map(0), "lean program nest deeper than 4 levels")
    # ... and moves an extended program to the LDS VM, which holds 6 (a seventh: test_limits_host.py)
    p = accepted(hp.nesting_spec(4), hp.nesting_map(0))
    assert p["X"] and not p["flat_top"]
    monkeypatch.setenv("MGX_NO_FLAT_TOP", "1")
    monkeypatch.setenv("MGX_NO_GEN", "1")
    assert not accepted(hp.nesting_spec(3), hp.nesting_map(0))["flat_top"]
    hp.run_parity("nest4_x", E, CHECK_ENVS)
    hp.run_parity("nest6_x", E, CHECK_ENVS)


def test_value_stack_and_query_depth_at_their_maximum():
    """A game value that needs all 8 stack entries (reward, observation value and GameValueFilter of every nesting
    scenario, lean and extended) and queries nested 3 levels (observation value, per-tick reward, event target); one
    more of either is refused by the compiler and by mgx_create (test_limits_host.py).  Queries are evaluated by the
    LDS VM only: programs whose action-phase handlers hold a query filter never take the register VM."""
    p = hp.create_one("query3")
    paths = p.paths
    p.close()
    assert paths["X"] and paths["rewards_ext"]
    hp.run_parity("query3", E, CHECK_ENVS)
