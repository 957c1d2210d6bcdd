"""The observation kernel only rewrites a row as far as the longer of its new and its previous token list (MgxDev::obs_used,
include/mgx.h mgx_set_buffers "OWNERSHIP"); the 0xFF padding behind that is what an earlier pass left in the bound buffer.

Every test runs two engines on the same maps, seeds and actions — one of them created under MGX_OBS_FULL_ROWS=1, which
rewrites whole rows in every pass like the reference does — and wants their observation buffers byte-equal, whatever
happened to the rows in between: rows growing and shrinking, episode restarts, a newly bound buffer full of other bytes,
envs loaded or copied over each other, the box output switched on and off, a caller scribbling into the buffer, token
overflow.  After a pass the engine's count of a row must be the index of the row's first 0xFF token."""
import os

import numpy as np
import pytest

from mettagrid_amd import engine, presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.fmt import K
from mettagrid_amd.mapgen import random_class_maps

pytestmark = pytest.mark.gpu

UNKNOWN = 0xFFFF
R3_OBJECTS, R3_AGENTS = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}


def _lean(n_maps, obs_tokens=200, max_steps=0):
    spec = presets.rung3_spec(obs_tokens=obs_tokens)
    spec.max_steps = max_steps
    prog = compile_spec(spec, 32, 32, max_objects=192)
    return prog, random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(n_maps))


def _rung4(n_maps, max_steps=0):
    prog = compile_spec(presets.rung4_spec(max_steps=max_steps), 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
    return prog, random_class_maps(prog, 64, 64, presets.RUNG4_OBJECTS, presets.RUNG4_AGENTS, range(n_maps))


def _pair(prog, cms, seeds):
    """(engine on the default path, engine that rewrites whole rows), device buffers."""
    tail = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    os.environ["MGX_OBS_FULL_ROWS"] = "1"
    try:
        full = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    finally:
        os.environ.pop("MGX_OBS_FULL_ROWS", None)
    assert (full.observation_counts() == UNKNOWN).all(), "MGX_OBS_FULL_ROWS keeps no counts"
    return tail, full


class _Actions:
    """Seeded action mixes: uniform over the action set, with stretches in which a random half of the agents only repeat
    action 0 (their rows then change little while the others' move on)."""

    def __init__(self, prog, E, seed):
        import torch
        self.torch, self.n, self.rows = torch, len(prog.action_names), E * prog.num_agents
        self.g = torch.Generator(device="cuda").manual_seed(seed)

    def next(self, t):
        torch = self.torch
        a = torch.randint(0, self.n, (self.rows,), dtype=torch.int32, device="cuda", generator=self.g)
        v = torch.randint(0, self.n, (self.rows,), dtype=torch.int32, device="cuda", generator=self.g)
        if (t // 10) % 3 == 2:
            idle = torch.rand(self.rows, device="cuda", generator=self.g) < 0.5
            a = torch.where(idle, torch.zeros_like(a), a)
        return a, v


def _step(engines, a, v):
    for eng in engines:
        eng.actions.copy_(a)
        eng.vibe_actions.copy_(v)
        eng.wait_for_caller()
        eng.step()
        eng.caller_waits()


def _first_pad(obs) -> np.ndarray:
    """Index of the first 0xFF 0xFF 0xFF token of every row (T: none), on the host."""
    o = obs.cpu().numpy()
    pad = (o == 0xFF).all(axis=2)
    return np.where(pad.any(axis=1), pad.argmax(axis=1), o.shape[1]).astype(np.uint16)


def _same(tail, full, where, counts=True):
    import torch
    tail.sync(); full.sync()
    if not torch.equal(tail.obs, full.obs):
        bad = (tail.obs != full.obs).any(dim=2).nonzero()[0].tolist()
        raise AssertionError(f"{where}: observation buffers differ, first at row {bad[0]} token {bad[1]}")
    assert torch.equal(tail.rewards, full.rewards) and torch.equal(tail.terminals, full.terminals) and \
        torch.equal(tail.truncations, full.truncations), where
    if counts:
        got, want = tail.observation_counts(), _first_pad(tail.obs)
        assert np.array_equal(got, want), f"{where}: counts differ from the first 0xFF token at rows {np.nonzero(got != want)[0][:8].tolist()}"
        return got.astype(np.int64)
    return None


class _Trend:
    """Did rows both grow and shrink between consecutive passes?"""

    def __init__(self, first):
        self.prev, self.grew, self.shrank = first, 0, 0

    def add(self, cur):
        self.grew += int((cur > self.prev).sum())
        self.shrank += int((cur < self.prev).sum())
        self.prev = cur

    def check(self, where):
        assert self.grew > 0 and self.shrank > 0, f"{where}: rows grew {self.grew} and shrank {self.shrank} times: the run proves nothing"


def _close(*engines):
    for e in engines:
        e.close()


def test_new_entry_points_are_exported():
    lib = engine.load_lib()   # (torch's HIP runtime first, like every other user of the library in this process)
    for name in ("mgx_invalidate_observations", "mgx_get_observation_counts"):
        assert name in engine.exported_symbols() and hasattr(lib, name), name
    assert lib.mgx_invalidate_observations(None) == -1 and lib.mgx_get_observation_counts(None, None) == -1


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_rows_grow_and_shrink(preset, E=24, steps=120):
    prog, cms = _lean(E) if preset == "lean" else _rung4(E)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 11)
    try:
        if preset == "lean":
            assert tail.obs_variant == 3 and full.obs_variant == 3, "the preset's instance of the observation kernel"
        trend = _Trend(_same(tail, full, f"{preset} initial observations"))
        acts = _Actions(prog, E, 3)
        for t in range(steps):
            _step((tail, full), *acts.next(t))
            trend.add(_same(tail, full, f"{preset} step {t + 1}"))
        trend.check(preset)
        assert tail.poll_errors()[0] == 0 and full.poll_errors()[0] == 0
    finally:
        _close(tail, full)


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_restarts_shorten_and_lengthen_rows(preset, E=24, steps=100):
    """Auto-reset on short episodes with a map pool: a restart keeps the rows and their counts, the initial observations of
    the new episode (another map) are then shorter or longer than what the old episode left."""
    n_maps = 7
    prog, maps = _lean(n_maps, max_steps=9) if preset == "lean" else _rung4(n_maps, max_steps=9)
    cms = maps[np.arange(E) % n_maps]
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 40)
    try:
        early = (np.arange(E, dtype=np.uint32) % 5) + 3   # the first episodes end at different steps: restarts in most steps
        for eng in (tail, full):
            eng.set_map_pool(maps)
            eng.set_auto_reset(True, pool_stride=3, early_end_steps=early)
        trend = _Trend(_same(tail, full, f"{preset} initial observations"))
        acts = _Actions(prog, E, 4)
        for t in range(steps):
            _step((tail, full), *acts.next(t))
            trend.add(_same(tail, full, f"{preset} auto-reset step {t + 1}"))
        trend.check(preset)
        assert int(tail.episodes()[0].min()) >= 5 and np.array_equal(tail.episodes()[0], full.episodes()[0])
        assert tail.poll_errors()[0] == 0 and full.poll_errors()[0] == 0
    finally:
        _close(tail, full)


def _rebind(eng, fill):
    """New caller buffers; the observation tensor starts out full of ``fill``."""
    import torch
    dev = eng.obs.device
    rows = eng.E * eng.A
    eng.obs = torch.full((rows, eng.T, 3), fill, dtype=torch.uint8, device=dev)
    eng.terminals = torch.zeros(rows, dtype=torch.bool, device=dev)
    eng.truncations = torch.zeros(rows, dtype=torch.bool, device=dev)
    eng.rewards = torch.zeros(rows, dtype=torch.float32, device=dev)
    eng.actions = torch.zeros(rows, dtype=torch.int32, device=dev)
    eng.vibe_actions = torch.zeros(rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng._bind(*(t.data_ptr() for t in (eng.obs, eng.terminals, eng.truncations, eng.rewards, eng.actions, eng.vibe_actions)), mem_kind=1)


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_rebinding_to_a_buffer_full_of_other_bytes(preset, E=12):
    prog, cms = _lean(E) if preset == "lean" else _rung4(E)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 5)
    try:
        acts = _Actions(prog, E, 6)
        for t in range(6):
            _step((tail, full), *acts.next(t))
        _same(tail, full, f"{preset} before the rebind")
        _rebind(tail, 0x5A)
        _rebind(full, 0xA5)
        _same(tail, full, f"{preset} initial observations in the new buffers")
        for t in range(6, 12):
            _step((tail, full), *acts.next(t))
            _same(tail, full, f"{preset} step {t + 1} after the rebind")
    finally:
        _close(tail, full)


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_loaded_and_copied_envs(preset, E=16):
    """An env with long rows over one with short rows and the other way round, by copy_envs and by save_envs / load_envs."""
    prog, cms = _lean(E) if preset == "lean" else _rung4(E)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 21)
    try:
        A = prog.num_agents
        acts = _Actions(prog, E, 8)
        for t in range(10):
            _step((tail, full), *acts.next(t))
        per_env = _same(tail, full, f"{preset} before the copy").reshape(E, A)
        order = np.argsort(per_env.sum(axis=1), kind="stable")
        short, short2, long2, long_ = int(order[0]), int(order[1]), int(order[-2]), int(order[-1])
        assert (per_env[long_] > per_env[short]).any() and (per_env[short2] < per_env[long2]).any()
        for eng in (tail, full):
            eng.copy_envs([long_, short2], [short, long2])   # long over short, short over long
        _same(tail, full, f"{preset} right after the copy", counts=False)
        unknown = tail.observation_counts().reshape(E, A)
        assert (unknown[[short, long2]] == UNKNOWN).all() and (unknown[[long_, short2]] != UNKNOWN).all()
        for t in range(10, 16):
            _step((tail, full), *acts.next(t))
            per_env = _same(tail, full, f"{preset} step {t + 1} after the copy").reshape(E, A)
        order = np.argsort(per_env.sum(axis=1), kind="stable")
        short, long_ = int(order[0]), int(order[-1])
        states = [(eng, eng.save_envs([long_, short])) for eng in (tail, full)]
        for t in range(16, 19):
            _step((tail, full), *acts.next(t))
        for eng, st in states:
            eng.load_envs(st, [short, long_])   # the saved long env into the short env's slot and the other way round
        _same(tail, full, f"{preset} right after the load", counts=False)
        for t in range(19, 25):
            _step((tail, full), *acts.next(t))
            _same(tail, full, f"{preset} step {t + 1} after the load")
        assert tail.poll_errors()[0] == 0 and full.poll_errors()[0] == 0
    finally:
        _close(tail, full)


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_scribble_then_invalidate(preset, E=12):
    import torch
    prog, cms = _lean(E) if preset == "lean" else _rung4(E)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 2)
    try:
        acts = _Actions(prog, E, 9)
        for t in range(5):
            _step((tail, full), *acts.next(t))
        _same(tail, full, f"{preset} before the scribble")
        for eng in (tail, full):
            eng.obs[:, eng.T // 3:, :] = 7    # a caller writes into the engine's buffer ...
            eng.obs[::2, :, 1] = 9
        tail.invalidate_observations()        # ... and says so
        assert (tail.observation_counts() == UNKNOWN).all()
        _step((tail, full), *acts.next(5))
        _same(tail, full, f"{preset} step behind the scribble")
        assert not bool((tail.obs[:, :, 0] == 7).any())
        for t in range(6, 10):
            _step((tail, full), *acts.next(t))
            _same(tail, full, f"{preset} step {t + 1}")
        torch.cuda.synchronize()
    finally:
        _close(tail, full)


@pytest.mark.parametrize("preset", ["lean", "rung4"])
def test_box_output_on_and_off(preset, E=12):
    """While the box output is on the token rows are not stored: rows and counts stay as they are and are still true when
    it is switched off again."""
    import torch
    prog, cms = _lean(E) if preset == "lean" else _rung4(E)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 30)
    try:
        acts = _Actions(prog, E, 10)
        for t in range(8):
            _step((tail, full), *acts.next(t))
        before = _same(tail, full, f"{preset} before the box output")
        rows_before = tail.obs.clone()
        shape = (E * prog.num_agents, len(prog.feature_norms), int(prog.words[K.H_OBS_HEIGHT]), int(prog.words[K.H_OBS_WIDTH]))
        boxes = [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(2)]
        for eng, box in zip((tail, full), boxes):
            eng.set_box_output(box)
        for t in range(8, 20):
            _step((tail, full), *acts.next(t))
        tail.sync(); full.sync()
        assert torch.equal(boxes[0], boxes[1]) and torch.equal(tail.obs, rows_before)
        assert np.array_equal(tail.observation_counts(), before)
        for eng in (tail, full):
            eng.set_box_output(None)
        for t in range(20, 26):
            _step((tail, full), *acts.next(t))
            _same(tail, full, f"{preset} step {t + 1}, box output off again")
    finally:
        _close(tail, full)


@pytest.mark.parametrize("T", [24, 22, 27])
def test_token_overflow(T, E=16, steps=40):
    """A token budget so small that rows overflow (the reference raises, the engine sets the env's error bit 1); T = 22 and
    27 also take the byte path of rows whose pitch 3 * T is not a multiple of four."""
    prog, cms = _lean(E, obs_tokens=T)
    tail, full = _pair(prog, cms, np.arange(E, dtype=np.uint32) + 17)
    try:
        got = _same(tail, full, f"T={T} initial observations")
        full_rows = int((got == T).sum())
        acts = _Actions(prog, E, 12)
        for t in range(steps):
            _step((tail, full), *acts.next(t))
            got = _same(tail, full, f"T={T} step {t + 1}")
            full_rows += int((got == T).sum())
        assert full_rows > 0, "no row ever filled up"
        bits_t, first_t = tail.poll_errors()
        bits_f, first_f = full.poll_errors()
        assert (bits_t, first_t) == (bits_f, first_f) and bits_t & 1, "token overflow: error bit 1 on both engines"
    finally:
        _close(tail, full)
