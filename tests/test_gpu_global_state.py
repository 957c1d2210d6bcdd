"""GPU: the global state rows (include/mgx.h mgx_set_global_state, csrc/mgx_global_state.h) — every env's objects as tokens,
written on the device behind every step — against the numpy restatement of the contract (mettagrid_amd/global_state.py
``expected_rows`` of the engine's own object records) bit for bit, and against what the REFERENCE's observations of the
committed goldens show at the same absolute cells."""
import glob
import json
import os

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
from mettagrid_amd import global_state as gs
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.fmt import K
from mettagrid_amd.mapgen import random_class_maps, random_map

pytestmark = pytest.mark.gpu
GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.npz"))
              if not os.path.basename(p).startswith("ref_"))  # ref_*: fixtures of test_reference_config.py
EMPTY = 0xFFFFFFFF
R3_OBJECTS, R3_AGENTS = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}


def host(eng):
    """(tokens u32 [E][TG], counts u32 [E], agent_start i32 [E][A] or None) of the engine's rows on the host."""
    eng.sync()
    t, c, s = eng.global_state
    return t.cpu().numpy(), c.cpu().numpy(), None if s is None else s.cpu().numpy()


def check_rows(eng, where, include=None, n_initial=None, envs=None):
    """Every (listed) env's row, count and agent starts equal ``expected_rows`` of the engine's own object records."""
    tok, cnt, start = host(eng)
    TG = tok.shape[1]
    envs = list(range(eng.E)) if envs is None else list(envs)
    for e, raw in zip(envs, eng.raw_objects_batch(envs)):
        n0 = None if n_initial is None else int(np.asarray(n_initial).reshape(-1)[e if np.size(n_initial) > 1 else 0])
        exp = gs.expected_rows(eng.prog, raw, include, n_initial=n0, max_tokens=TG)
        assert int(cnt[e]) == exp.count, f"{where}: env {e} counts {int(cnt[e])}, expected {exp.count}"
        if not np.array_equal(tok[e], exp.tokens):
            k = int(np.argmax(tok[e] != exp.tokens))
            raise AssertionError(f"{where}: env {e} token {k} of {exp.count} (TG {TG}): {int(tok[e, k]):#010x}, expected {int(exp.tokens[k]):#010x}")
        assert (tok[e, min(exp.count, TG):] == EMPTY).all()
        if start is not None:
            assert np.array_equal(start[e], exp.agent_start), f"{where}: env {e} agent_start {start[e].tolist()} vs {exp.agent_start.tolist()}"
    return tok, cnt, start


def step_random(eng, rng):
    import torch
    n, rows = len(eng.prog.action_names), eng.E * eng.A
    eng.actions.copy_(torch.as_tensor(rng.integers(0, n, rows).astype(np.int32), device=eng.actions.device))
    eng.vibe_actions.copy_(torch.as_tensor(rng.integers(0, n, rows).astype(np.int32), device=eng.actions.device))
    eng.wait_for_caller()
    eng.step()
    eng.caller_waits()


def rung3(E, max_steps=0):
    spec = presets.rung3_spec()
    spec.max_steps = max_steps
    prog = compile_spec(spec, 32, 32, max_objects=192)
    return prog, random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(E))


# ---- 3. golden replay, every step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_golden_replay_every_step(path):
    import torch
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    spec = hp.SCENARIOS[meta["scenario"]][0]()
    cm, ref_obs, actions, vibe_actions = z["class_map"], z["obs"], z["actions"], z["vibe_actions"]   # (each read inflates the array)
    prog = hp.compile_scenario(meta["scenario"], spec, *cm.shape)
    eng = BatchedMettaGrid(prog, cm[None], [meta["seed"]], buffers="device", specialize=False)
    tokens, counts, starts = eng.set_global_state()
    assert tokens.shape == (1, eng.global_state_bound()) and tokens.dtype == torch.uint32
    n_initial = int((cm != 0).sum())
    name = os.path.basename(path)[:-4]

    def check(t):
        tok, cnt, start = check_rows(eng, f"{name} step {t}", n_initial=n_initial)
        assert int(cnt[0]) <= tok.shape[1], "global_state_bound is no bound"
        groups = {(r, c): fv for r, c, fv in gs.split_row(tok[0])}
        for a in range(prog.num_agents):   # what the REFERENCE showed this agent at this step
            first = int(tok[0, start[0, a]])
            for r, c, fv in gs.from_observation(ref_obs[t][a], first & 0xFF, (first >> 8) & 0xFF, prog):
                assert groups.get((r, c)) == fv, f"{name} step {t}: the reference shows agent {a} {fv} at ({r}, {c}), the row holds {groups.get((r, c))}"
    check(0)
    for t in range(meta["steps"]):
        eng.actions.copy_(torch.as_tensor(actions[t], device="cuda"))
        eng.vibe_actions.copy_(torch.as_tensor(vibe_actions[t], device="cuda"))
        eng.wait_for_caller()
        eng.step()
        check(t + 1)
    assert eng.poll_errors()[0] == 0
    assert np.array_equal(eng.obs.cpu().numpy(), ref_obs[-1])   # (the replay is the golden's)
    eng.close()


# ---- 4. shapes where the kernel can go wrong -------------------------------------------------------------------------------
def small_map(seed):   # H * W = 54 < 64: one partial chunk
    return random_map(6, 9, {"wall": 3, "extractor": 3, "chest": 2}, {"red": 3, "blue": 2}, seed)


SHAPES = {
    "rung3_E70": lambda: rung3(70),                                     # > 64 envs, a partial last workgroup (70 = 17 * 4 + 2)
    "keyhole_7x10": lambda: _scenario("keyhole", hp.keyhole_map, 3),    # H * W = 70: one full chunk + 6 cells
    "letterbox_9x12": lambda: _scenario("letterbox", hp.letterbox_map, 3),   # H * W = 108
    "small_6x9": lambda: _scenario("keyhole", small_map, 3),            # H * W = 54 < 64
    "rung4_E5": lambda: _scenario("rung4", hp.rung4_map, 5),            # the extended state: dynamic tags, flags
}


def _scenario(name, map_f, E):
    spec = hp.SCENARIOS[name][0]()
    cells = [map_f(s) for s in range(E)]
    prog = hp.compile_scenario(name, spec, *cells[0].shape)
    return prog, np.stack([prog.class_map(c) for c in cells])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(shape):
    prog, cms = SHAPES[shape]()
    E = cms.shape[0]
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32) + 11, buffers="device", specialize=False)
    eng.set_global_state()
    n_initial = (cms.reshape(E, -1) != 0).sum(axis=1)
    rng = np.random.default_rng(5)
    check_rows(eng, f"{shape} step 0", n_initial=n_initial)
    for t in range(12):
        step_random(eng, rng)
        if t in (0, 11):
            check_rows(eng, f"{shape} step {t + 1}", n_initial=n_initial)
    assert eng.poll_errors()[0] == 0
    eng.close()


# ---- 5. overflow -----------------------------------------------------------------------------------------------------------
def test_overflow_stays_inside_the_row():
    import torch
    E = 3
    prog, cms = rung3(E)
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    full = [gs.expected_rows(prog, raw) for raw in eng.raw_objects_batch(range(E))]
    TG = full[1].count - 3
    GUARD, SENT = 64, 0x5A5A5A5A
    flat = torch.full((GUARD + E * TG + GUARD,), SENT, dtype=torch.int32, device="cuda").view(torch.uint32)
    counts = torch.zeros(E, dtype=torch.int32, device="cuda").view(torch.uint32)
    starts = torch.full((E, prog.num_agents), -7, dtype=torch.int32, device="cuda")
    eng.bind_global_state(flat[GUARD:GUARD + E * TG].view(E, TG), counts, starts)
    rng = np.random.default_rng(2)
    for t in range(3):
        tok, cnt, start = check_rows(eng, f"overflow step {t}")
        assert np.array_equal(tok[1], full[1].tokens[:TG]) or t > 0
        assert cnt[1] > TG or t > 0                                # counts is the full number ...
        f = flat.cpu().numpy()
        assert (f[:GUARD] == SENT).all() and (f[-GUARD:] == SENT).all()   # ... and nothing is stored outside the rows
        step_random(eng, rng)
    # An agent that starts at or behind TG has agent_start -1.  The maps end in a border wall row, so with TG = count - 3 no
    # agent starts that late; the same engine with a second, shorter TG: exactly at the start of env 1's last agent (that
    # agent starts AT TG), and one token further on (the agent's first token fits, its start is reported).
    exp = gs.expected_rows(prog, eng.raw_objects(1))
    for TG2, hidden in ((int(exp.agent_start.max()), 1), (int(exp.agent_start.max()) + 1, 0)):
        flat.view(torch.int32).fill_(SENT)
        eng.bind_global_state(flat[GUARD:GUARD + E * TG2].view(E, TG2), counts, starts)
        tok, cnt, start = check_rows(eng, f"overflow TG {TG2}")
        assert (start[1] == -1).sum() == hidden and (start[1] < TG2).all() and cnt[1] == exp.count > TG2
        f = flat.cpu().numpy()
        assert (f[:GUARD] == SENT).all() and (f[GUARD + E * TG2:] == SENT).all()
    for bad in (0, -5):
        with pytest.raises(ValueError, match="row length"):
            engine_check(eng, eng.L.mgx_set_global_state(eng.h, flat.data_ptr(), bad, counts.data_ptr(), None, None))
    check_rows(eng, "a refused call changes nothing")
    eng.close()


def engine_check(eng, rc):
    from mettagrid_amd.engine import _check
    _check(rc)


def test_host_buffer_engines_are_refused():
    prog, cms = rung3(1)
    eng = BatchedMettaGrid(prog, cms, [1], buffers="host", specialize=False)
    with pytest.raises(ValueError, match="host buffers"):
        eng.set_global_state()
    import torch
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="host buffers"):
        engine_check(eng, eng.L.mgx_set_global_state(eng.h, t.data_ptr(), 64, t.data_ptr(), None, None))
    with pytest.raises(ValueError, match="no rows set"):
        eng.write_global_state()
    eng.close()


# ---- 6. shrinking rows -----------------------------------------------------------------------------------------------------
def test_shrinking_rows_and_masked_rewrite():
    import torch
    E = 6
    prog, cms = rung3(E)
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    tokens, counts, starts = eng.set_global_state()
    before, cnt_before, _ = check_rows(eng, "before")
    fewer = random_class_maps(prog, 32, 32, {"wall": 3, "extractor": 1, "chest": 1}, R3_AGENTS, range(E))
    mask = np.zeros(E, np.uint8)
    mask[[1, 4]] = 1
    eng.reset_envs(mask, fewer, np.arange(E, dtype=np.uint32) + 100)
    eng.sync()
    SENT = 0x12345678
    keep = [0, 2, 3, 5]
    tokens.view(torch.int32)[keep] = SENT   # (uint32 tensors have no indexed stores)
    torch.cuda.synchronize()
    eng.write_global_state([1, 4])
    tok, cnt, _ = check_rows(eng, "after the masked rewrite", envs=[1, 4])
    assert (cnt[[1, 4]] < cnt_before[[1, 4]]).all()
    for e in (1, 4):   # the old tail is gone
        assert (tok[e, cnt[e]:cnt_before[e]] == EMPTY).all() and (tok[e, cnt[e]:] == EMPTY).all()
    assert (tok[keep] == SENT).all() and np.array_equal(cnt[keep], cnt_before[keep])   # unmasked rows: not touched
    eng.close()


# ---- 7. filter -------------------------------------------------------------------------------------------------------------
def test_class_filter():
    E = 4
    prog, cms = rung3(E)
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    rng = np.random.default_rng(3)
    inc = gs.class_include(prog, ["wall"])
    tokens, _, _ = eng.set_global_state(exclude=["wall"])
    assert tokens.shape[1] == eng.global_state_bound(["wall"]) <= eng.global_state_bound()
    for t in range(3):
        tok, cnt, start = check_rows(eng, f"no walls, step {t}", include=inc)
        assert (start >= 0).all()
        step_random(eng, rng)
    everything = list(range(len(inc)))
    eng.set_global_state(exclude=everything)
    for t in range(2):
        tok, cnt, start = check_rows(eng, f"nothing, step {t}", include=np.zeros(len(inc), np.uint8))
        assert (cnt == 0).all() and (tok == EMPTY).all() and (start == -1).all()
        step_random(eng, rng)
    eng.close()


# ---- 8. derived state ------------------------------------------------------------------------------------------------------
def test_copy_envs_then_write():
    E = 5
    prog, cms = rung3(E)
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    eng.set_global_state()
    rng = np.random.default_rng(4)
    for _ in range(5):
        step_random(eng, rng)
    eng.copy_envs([0, 3], [2, 4])
    eng.set_inventory(1, 0, {0: 7})
    eng.write_global_state([1, 2, 4])
    tok, cnt, start = check_rows(eng, "after copy_envs")
    assert np.array_equal(tok[2], tok[0]) and np.array_equal(tok[4], tok[3]) and cnt[2] == cnt[0] and np.array_equal(start[4], start[3])
    eng.close()


def test_wrapper_with_map_pool_and_auto_reset():
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    E, M = 6, 4
    spec = presets.rung3_spec()
    spec.max_steps = 5
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    pool = random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(M))
    pool[1:] = random_class_maps(prog, 32, 32, {"wall": 9, "extractor": 3, "chest": 2}, R3_AGENTS, range(1, M))   # rows shrink and grow
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, buffers="device", specialize=False, global_state=True,
                              global_state_exclude=(), episode_stats=False)
    env.reset()
    eng = env.engine
    assert env.global_state is eng.global_state and env.global_state[0].shape == (E, eng.global_state_bound())
    check_rows(eng, "wrapper reset")
    g = torch.Generator(device="cuda").manual_seed(1)
    ends = 0
    for t in range(13):
        a = torch.randint(0, env.transport_action_n, (env.num_agents,), dtype=torch.int32, device="cuda", generator=g)
        _, _, term, trunc, _ = env.step(a)
        check_rows(eng, f"wrapper step {t + 1}")    # (a finished env: its final state; the next step: the new map after one tick)
        ends += int(bool(trunc.all()))
    assert ends >= 2
    st = env.save_state([0])
    env.step(torch.zeros(env.num_agents, dtype=torch.int32, device="cuda"))
    env.load_state(st, [5])
    tok, _, _ = check_rows(eng, "wrapper load_state")
    env.close()


def test_parallel_env_state():
    from mettagrid_amd.envs import MettaGridParallelEnv
    spec = presets.rung2_spec()
    cells = presets.rung2_map(3)
    plain = MettaGridParallelEnv(spec, cells, seed=1)
    env = MettaGridParallelEnv(spec, cells, seed=1, global_state=True, global_state_exclude=["wall"])
    obs, _ = env.reset()
    pobs, _ = plain.reset()
    for t in range(3):
        acts = {a: (a + t) % env.action_space_n(a) for a in env.agents}
        out, pout = env.step(acts), plain.step(acts)
        assert all(np.array_equal(out[0][a], pout[0][a]) for a in env.agents) and out[1] == pout[1]
        s = env.state()
        b = env._sim._b
        exp = gs.expected_rows(b.prog, b.raw_objects(0), gs.class_include(b.prog, ["wall"]), max_tokens=s.shape[0])
        assert s.dtype == np.uint8 and s.shape[1] == 4 and np.array_equal(s.reshape(-1).view(np.uint32), exp.tokens)
    assert not plain.state().any()   # the default stays the reference's stub
    env.close(); plain.close()


# ---- 9. off means off ------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """An engine that never set the feature and one that set and unset it step exactly like the CPU oracle (the behaviour
    before this feature) and like an engine that keeps it on: observations, rewards and state digests over 20 steps.  That
    nothing is enqueued while it is off is one ``if (e->gs_on)`` in mgx_step, as for the step stats."""
    E = 8
    prog, cms = rung3(E)
    seeds = np.arange(E, dtype=np.uint32) + 40
    never, toggled, on = (BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False) for _ in range(3))
    toggled.set_global_state()
    assert toggled.set_global_state(max_tokens=0) is None and toggled.global_state is None and never.global_state is None
    on.set_global_state(exclude=["wall"])
    oracle = op.OracleSim(prog, cms[0], int(seeds[0]))
    oracle.reinit_buffers()
    rng = np.random.default_rng(9)
    A, n = prog.num_agents, len(prog.action_names)
    import torch
    for t in range(20):
        a, v = rng.integers(0, n, E * A).astype(np.int32), rng.integers(0, n, E * A).astype(np.int32)
        for eng in (never, toggled, on):
            eng.actions.copy_(torch.as_tensor(a, device="cuda"))
            eng.vibe_actions.copy_(torch.as_tensor(v, device="cuda"))
            eng.wait_for_caller()
            eng.step()
            eng.sync()
        oracle.step(a[:A], v[:A])
        ref = oracle.snapshot()
        assert np.array_equal(never.obs.cpu().numpy()[:A], ref["obs"]) and np.array_equal(never.rewards.cpu().numpy()[:A], ref["rewards"])
        d = never.state_digests()
        for eng in (toggled, on):
            assert torch.equal(eng.obs, never.obs) and torch.equal(eng.rewards, never.rewards), f"step {t}"
            assert np.array_equal(eng.state_digests(), d), f"step {t}"
    for eng in (never, toggled, on):
        eng.close()
