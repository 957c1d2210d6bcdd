"""GPU: the three host-driven restarts (include/mgx.h mgx_reset_envs, mgx_reset_envs_from_pool, mgx_reset_envs_generated)
called directly on bound buffers: the restarted envs' caller rows equal a fresh engine's, every other row stays as it was."""
import numpy as np
import pytest

import mapgen_cases as mc
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import generated_class_maps

pytestmark = pytest.mark.gpu

E = 5
MASK = np.array([1, 1, 0, 1, 0], np.uint8)   # a run of two envs, a single env, untouched envs between and behind them
ROWS = ("obs", "terminals", "truncations", "rewards")
SEEDS0 = np.arange(E, dtype=np.uint32) * 7 + 3
NEW_SEEDS = np.array([101, 202, 303, 404, 505], np.uint32)
MAP_SEEDS0 = [11, 12, 13, 14, 15]
NEW_MAP_SEEDS = np.array([4000000001, 21, 22, 2 ** 31, 24], np.uint32)
POOL_SEEDS = [31, 32, 33]
POOL_INDEX = np.array([2, 0, 1, 1, 0], np.int32)


def _rows(eng):
    """The caller-visible rows as numpy [E, A, ...] copies."""
    get = (lambda a: a.copy()) if eng.kind == "host" else (lambda t: t.cpu().numpy())
    eng.sync()
    return {k: get(getattr(eng, k)).reshape((E, eng.A) + getattr(eng, k).shape[1:]) for k in ROWS}


def _step(eng, actions):
    if eng.kind == "host":
        eng.actions[:] = actions
    else:
        import torch
        eng.actions.copy_(torch.as_tensor(actions).cuda())
        torch.cuda.synchronize()
    eng.step()


def _equal(a, b, envs, what):
    for k in ROWS:
        assert np.array_equal(a[k][envs], b[k][envs]), f"{what}: '{k}' differs"


@pytest.mark.parametrize("buffers", ["host", "device"])
@pytest.mark.parametrize("path", ["maps", "pool", "generated"])
def test_direct_restart_equals_a_fresh_engine(path, buffers):
    """Rung-3 rules with all 16 agents on the 32 x 32 recipe of mapgen_cases (the smallest one that places them all on a square
    map).  (a) restarted envs = a fresh host-buffer engine on their maps and seeds, (b) the others unchanged, (c) both still
    hold two steps later, the others then equal a twin that was never restarted; an all-zero mask changes nothing."""
    prog, spec = mc.case(900, 1, True)
    A = prog.num_agents
    maps0 = generated_class_maps(spec, prog, MAP_SEEDS0)
    pool = generated_class_maps(spec, prog, POOL_SEEDS)
    new_maps = pool[POOL_INDEX] if path == "pool" else generated_class_maps(spec, prog, NEW_MAP_SEEDS)
    acts = np.random.RandomState(5).randint(0, len(prog.action_names), (5, E * A)).astype(np.int32)

    eng = BatchedMettaGrid(prog, maps0, SEEDS0, buffers=buffers)
    twin = BatchedMettaGrid(prog, maps0, SEEDS0, buffers=buffers)
    fresh = BatchedMettaGrid(prog, new_maps, NEW_SEEDS, buffers="host")
    if path == "pool":
        eng.set_map_pool(pool)
    elif path == "generated":
        eng.set_map_generator(spec, 0)

    def restart(mask):
        if path == "maps":
            eng.reset_envs(mask, new_maps, NEW_SEEDS)
        elif path == "pool":
            eng.reset_envs_from_pool(mask, POOL_INDEX, NEW_SEEDS)
        else:
            eng.reset_envs_generated(mask, NEW_MAP_SEEDS, NEW_SEEDS)

    for t in range(3):
        _step(eng, acts[t])
        _step(twin, acts[t])
    before = _rows(eng)
    m = MASK.astype(bool)
    restart(np.zeros(E, np.uint8))
    _equal(_rows(eng), before, slice(None), "all-zero mask")
    restart(MASK)
    _equal(_rows(eng), _rows(fresh), m, "(a) restarted envs")
    _equal(_rows(eng), before, ~m, "(b) other envs")
    for t in (3, 4):
        for e in (eng, twin, fresh):
            _step(e, acts[t])
    _equal(_rows(eng), _rows(fresh), m, "(c) restarted envs")
    _equal(_rows(eng), _rows(twin), ~m, "(c) other envs")
    for e in (eng, twin, fresh):
        e.close()
