"""The staging front of the observation kernel (mgx_obs.h phase 0a / 0b: every first-level load of a thread issued into
registers, the dependent loads behind one wait, then the LDS writes) on the shapes the other suites do not reach: a grid
that is not a whole number of 16-byte loads with fewer agents than a DPP row, a grid that needs a second pass of the grid
loop, more object slots than threads (the classification loop behind the first barrier, whose first pass is the hoisted
one), and the rung-3 preset on the generic instance beside the specialised one.  (An empty pool prefix has no case: the
compiler gives every class its `type:` tag, as the reference does, so no compiled program has a class without tag tokens.)

Every case runs a handful of envs for six steps from step 0 and wants every env's caller-visible buffers equal to the
oracle's after construction and after every step (helpers.compare_snapshots), and no error bit."""
import os

import numpy as np
import pytest

import helpers
import oracle_py
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_map

pytestmark = pytest.mark.gpu

E, STEPS = 5, 6
R3_OBJECTS, R3_AGENTS = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}


def _small():
    """7 x 9 cells = 126 bytes of grid: seven 16-byte loads and a ragged tail of seven cells; three agents."""
    spec = helpers.teams_spec(presets.rung3_spec(), 3, 2)
    maps = [random_map(7, 9, {"wall": 3, "extractor": 3, "chest": 2}, {"red": 2, "blue": 1}, 50 + s) for s in range(E)]
    return compile_spec(spec, 7, 9, max_objects=48), maps


def _wide():
    """48 x 48 cells = 288 16-byte loads: the grid loop's second pass behind the hoisted first one."""
    maps = [random_map(48, 48, R3_OBJECTS, R3_AGENTS, 60 + s) for s in range(E)]
    return compile_spec(presets.rung3_spec(), 48, 48, max_objects=256), maps


def _many_slots():
    """320 object slots on a 16 x 16 map: more slots than the workgroup has threads."""
    maps = [random_map(16, 16, {"wall": 12, "extractor": 6, "chest": 3}, R3_AGENTS, 70 + s) for s in range(E)]
    return compile_spec(presets.rung3_spec(), 16, 16, max_objects=320), maps


def _preset():
    maps = [presets.rung3_map(90 + s) for s in range(E)]
    return compile_spec(presets.rung3_spec(), 32, 32, max_objects=192), maps


def _engine(prog, cms, seeds, **env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return BatchedMettaGrid(prog, cms, seeds, buffers="host", specialize=False)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(prog, maps, engines, where):
    """Steps ``engines`` and one oracle per env side by side; every env of every engine against its oracle, every step."""
    A = prog.num_agents
    cms = np.stack([prog.class_map(m) for m in maps])
    seeds = np.arange(E, dtype=np.uint32) * 5 + 1
    engs = [make(prog, cms, seeds) for make in engines]
    try:
        oracles = [oracle_py.OracleSim(prog, cms[i], int(seeds[i])) for i in range(E)]
        for o in oracles:
            o.reinit_buffers()
        acts = [helpers.make_actions(prog, 300 + i, STEPS, False) for i in range(E)]
        snaps = []
        for t in range(STEPS + 1):
            if t > 0:
                for eng in engs:
                    eng.actions[:] = np.concatenate([acts[i][0][t - 1] for i in range(E)])
                    eng.vibe_actions[:] = np.concatenate([acts[i][1][t - 1] for i in range(E)])
                    eng.step()
                for i, o in enumerate(oracles):
                    o.step(acts[i][0][t - 1], acts[i][1][t - 1])
            snaps = [eng.snapshot() for eng in engs]
            for i, o in enumerate(oracles):
                want = o.snapshot()
                for n, snap in enumerate(snaps):
                    helpers.compare_snapshots(want, {k: v[i * A:(i + 1) * A] for k, v in snap.items()},
                                              f"{where} engine {n} env {i} step {t}")
            for snap in snaps[1:]:   # the engines against each other, byte for byte
                for k in ("obs", "rewards", "terminals", "truncations"):
                    assert np.array_equal(snaps[0][k], snap[k]), f"{where} step {t}: '{k}' differs between the engines"
        for eng in engs:
            assert eng.poll_errors()[0] == 0, where
        return engs, snaps
    except BaseException:
        for eng in engs:
            eng.close()
        raise


def _close(engs):
    for eng in engs:
        eng.close()


def test_ragged_grid_and_three_agents():
    prog, maps = _small()
    assert (7 * 9 * 2) % 16 != 0 and prog.num_agents == 3
    engs, _ = _run(prog, maps, [_engine], "7x9")
    _close(engs)


def test_second_pass_of_the_grid_loop():
    prog, maps = _wide()
    assert 48 * 48 * 2 // 16 > 256
    engs, _ = _run(prog, maps, [_engine], "48x48")
    _close(engs)


def test_more_object_slots_than_threads():
    prog, maps = _many_slots()
    assert prog.max_objects > 256
    engs, _ = _run(prog, maps, [_engine], "320 slots")
    _close(engs)


def test_preset_on_the_generic_instance():
    prog, maps = _preset()
    engs, _ = _run(prog, maps, [_engine, lambda p, c, s: _engine(p, c, s, MGX_OBS_GENERIC="1")], "rung-3 preset")
    try:
        assert (engs[0].obs_variant, engs[1].obs_variant) == (3, 0), "the specialised instance beside the generic one"
    finally:
        _close(engs)
