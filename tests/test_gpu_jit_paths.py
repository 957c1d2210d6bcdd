"""GPU: state that survives the switch to run-time specialised kernels (mettagrid_amd/jit.py, mgx_attach_code) and the engine
calls made after it.  Two programs whose code objects tests/test_gpu_jit_matrix.py compiles: `torture` (world + observation,
on_tick handlers, episodes of 40 steps) and `window15` (observation only, rows that fill the whole token budget).  Every case
runs 45 envs and compares a specialised engine or env with a `specialize=False` twin after every step, bit for bit."""
import numpy as np
import pytest

import jit_cases as jc

pytestmark = pytest.mark.gpu
E = jc.E_MATRIX
PROGRAMS = ("torture", "window15")


@pytest.fixture(scope="module", autouse=True)
def compiled():
    jc.wait_for(PROGRAMS)
    with jc.cache_env():
        yield


def _how(name: str) -> str:
    return "sync" if jc.case(name).world else "obs"


def _assert_attached(eng, name: str) -> None:
    want = (9, 9, 9) if jc.case(name).world else (0, 0, 9)
    got = (eng.handler_variant, eng.world_variant, eng.obs_variant)
    assert got == want and getattr(eng, "jit_errors", []) == [] and getattr(eng, "attach_rc", 0) == 0, (name, got, eng.jit_errors)


def _twin(name: str, **kw) -> "jc.Twin":
    tw = jc.Twin(jc.case(name), E, _how(name), **kw)
    try:
        _assert_attached(tw.spec, name)
    except BaseException:
        tw.close()
        raise
    return tw


@pytest.mark.parametrize("name", PROGRAMS)
def test_attach_in_the_middle_of_an_episode(name):
    """The production "async" hand-over: both engines start generic, one gets its code objects between steps 7 and 8."""
    tw = jc.Twin(jc.case(name), E, False)
    try:
        for _ in range(7):
            tw.step()
        assert (tw.spec.handler_variant, tw.spec.world_variant, tw.spec.obs_variant) == (0, 0, 0)
        if jc.case(name).world:
            tw.spec._start_jit(wait=True)
        else:
            assert jc.attach_obs(tw.spec, tw.c) == 0, tw.spec.attach_error
        tw.step()
        _assert_attached(tw.spec, name)
        assert tw.plain.obs_variant == 0 and tw.plain.handler_variant == 0
        for _ in range(25):
            tw.step()
        tw.finish()
    finally:
        tw.close()


def _rebind(eng, fill: int) -> dict:
    """Fresh caller buffers (observations full of ``fill``); the old ones are returned."""
    import torch
    old = {k: getattr(eng, k) for k in ("obs", "terminals", "truncations", "rewards", "actions", "vibe_actions")}
    rows, dev = eng.E * eng.A, eng.obs.device
    eng.obs = torch.full((rows, eng.T, 3), fill, dtype=torch.uint8, device=dev)
    eng.terminals = torch.zeros(rows, dtype=torch.bool, device=dev)
    eng.truncations = torch.zeros(rows, dtype=torch.bool, device=dev)
    eng.rewards = torch.zeros(rows, dtype=torch.float32, device=dev)
    eng.actions = torch.zeros(rows, dtype=torch.int32, device=dev)
    eng.vibe_actions = torch.zeros(rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng._bind(*(t.data_ptr() for t in (eng.obs, eng.terminals, eng.truncations, eng.rewards, eng.actions, eng.vibe_actions)), mem_kind=1)
    return old


@pytest.mark.parametrize("name", PROGRAMS)
def test_rebinding_buffers_after_attach(name):
    """mgx_set_buffers under attached code objects: the world code object reads the buffer addresses from its own MgxDev copy
    in module constant memory (refreshed when the host table differs), the observation one from the launch arguments."""
    import torch
    tw = _twin(name)
    try:
        for _ in range(6):
            tw.step()
        old = _rebind(tw.spec, 0x5A)
        _rebind(tw.plain, 0xA5)   # (mgx_set_buffers starts the flag and reward rows afresh: on both sides, to stay twins)
        for o in tw.oracles.values():
            o.reinit_buffers()    # (the reference's set_buffers: episode rewards start again)
        kept = {k: v.clone() for k, v in old.items() if k not in ("actions", "vibe_actions")}
        jc.same_everywhere(tw.spec, tw.plain, f"{name}: initial observations in the new buffers", tw.envs)
        assert not (tw.spec.obs == 0x5A).all(dim=2).all(dim=1).any(), "a row of the new observation tensor was not written"
        for _ in range(8):
            tw.step()
            for k, v in kept.items():
                assert torch.equal(old[k], v), f"{name}: the old '{k}' tensor was written after the rebind (step {tw.t})"
        assert tw.spec.obs.data_ptr() != old["obs"].data_ptr() and not torch.equal(tw.spec.obs, old["obs"])
        _assert_attached(tw.spec, name)
        tw.finish()
    finally:
        tw.close()


@pytest.mark.parametrize("name", PROGRAMS)
def test_dense_output_on_and_off_after_attach(name):
    """While dense output is on the engine leaves the observation code object (it has token-row kernels only) without a word;
    switched off again, the code object writes token rows whose written-token counts (MgxDev::obs_used) it shares with the
    generic kernel that ran in between."""
    import torch
    from mettagrid_amd.fmt import K
    tw = _twin(name, with_oracle=False)   # (the oracle's token rows have no counterpart while the box is on)
    try:
        for _ in range(5):
            tw.step()
        prog = tw.c.prog
        shape = (E * tw.A, len(prog.feature_norms), int(prog.words[K.H_OBS_HEIGHT]), int(prog.words[K.H_OBS_WIDTH]))
        boxes = [torch.full(shape, float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for g, b in zip((tw.spec, tw.plain), boxes):
            g.set_box_output(b)
        for _ in range(6):
            tw.step()   # (token rows: stale on both sides)
            assert torch.equal(boxes[0], boxes[1]) and not torch.isnan(boxes[0]).any(), f"{name}: boxes differ at step {tw.t}"
        stale = tw.spec.obs.clone()
        for g in (tw.spec, tw.plain):
            g.set_box_output(None)
        for _ in range(6):
            tw.step()   # token rows again, compared in full
        assert not torch.equal(tw.spec.obs, stale)
        _assert_attached(tw.spec, name)
        tw.finish()
    finally:
        tw.close()


@pytest.mark.parametrize("name", PROGRAMS)
def test_restart_onto_denser_maps_after_attach(name):
    """mgx_reset_envs with maps that hold more objects than any map at create: the observation kernel's LDS token pool grows
    under the attached code object (grow_pool re-plans the LDS and keeps obs_variant 9 while the kernel fits 64 KiB)."""
    from mettagrid_amd.engine import BatchedMettaGrid
    c = jc.case(name)
    sparse = np.stack([c.prog.class_map(jc.SPARSE[name](s)) for s in range(E)])
    envs = list(jc.DENSE_ENVS)
    dense = [c.prog.class_map(jc.DENSE[name](700 + k)) for k in range(len(envs))]
    tw = _twin(name, cms=sparse)
    fresh = None
    try:
        pool0 = tw.spec.env_state_info()["pool_tokens"]
        for _ in range(jc.DENSE_AT):
            tw.step()
        tw.reset(envs, maps=dense)
        assert tw.spec.env_state_info()["pool_tokens"] > pool0, "the maps were not dense enough to grow the token pool"
        assert tw.spec.obs_variant == 9, "these small programs fit 64 KiB after the growth"
        fresh = BatchedMettaGrid(c.prog, tw.cms[envs], tw.seeds[envs], buffers="device", specialize=False)
        A = tw.A
        rows = np.concatenate([np.arange(i * A, (i + 1) * A) for i in envs])

        def against_fresh(where):
            a, b = tw.spec.snapshot(), fresh.snapshot()
            for k in a:
                assert np.array_equal(a[k][rows], b[k]), f"{name} {where}: '{k}' differs from a fresh engine on the dense maps"
            assert np.array_equal(tw.spec.state_digests()[envs], fresh.state_digests())

        against_fresh("after the restart")
        assert tw.spec.poll_errors()[0] == 0   # (past a token overflow the token statistics of a restart mean nothing)
        for _ in range(jc.DENSE_STEPS - jc.DENSE_AT):
            a, v = tw.acts.next()
            jc.step_engines((tw.spec, tw.plain), a, v)
            jc.step_engines((fresh,), a[rows], v[rows])
            for i, o in tw.oracles.items():
                o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
            tw.t += 1
            tw.check(f"step {tw.t} (dense maps)")
            against_fresh(f"step {tw.t}")
        _assert_attached(tw.spec, name)
        tw.finish()
        assert fresh.poll_errors()[0] == 0
    finally:
        tw.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("name", PROGRAMS)
def test_env_state_across_specialised_and_generic_engines(name):
    """save_envs from the specialised engine into the generic one and the other way round, copy_envs inside each, then 10
    steps.  (No oracle: the envs are moved about.)"""
    tw = _twin(name, with_oracle=False)
    try:
        for _ in range(8):
            tw.step()
        moved = [3, 31, 32, 40]
        from_spec, from_plain = tw.spec.save_envs(moved), tw.plain.save_envs(moved)
        for _ in range(4):
            tw.step()
        tw.plain.load_envs(from_spec)            # back to step 8, each from the OTHER engine's records
        tw.spec.load_envs(from_plain)
        tw.check("after load_envs across the engines")
        for g in (tw.spec, tw.plain):
            g.copy_envs([0, 33, 3], [5, 44, 33])   # across the wavefront boundary, a loaded env among the sources
        tw.check("after copy_envs")
        some = tw.spec.save_envs([5, 44])
        tw.plain.load_envs(some, [6, 43])
        tw.spec.load_envs(some, [6, 43])
        tw.check("after loading the specialised engine's records into other slots")
        for _ in range(10):
            tw.step()
        _assert_attached(tw.spec, name)
        tw.finish()
    finally:
        tw.close()


def test_two_specialised_engines_of_one_program_alive_at_once():
    """Each attached world code object is a module of its own, with its own g_mgx_dev in constant memory: two engines of one
    program (other maps, seeds and actions) stepped alternately, each equal to its twin."""
    one = _twin("torture")
    two = None
    try:
        two = _twin("torture", action_seed=99, seed0=1001, cms=jc.class_maps(jc.case("torture"), range(300, 300 + E)))
        for _ in range(20):
            one.step()
            two.step()
        one.finish()
        two.finish()
    finally:
        one.close()
        if two is not None:
            two.close()


def _same_struct(a, b, where: str) -> None:
    """Two nested structures of dicts, sequences, arrays and scalars are equal: same keys and lengths, arrays and numbers bit
    for bit (NaN equal to NaN)."""
    assert type(a) is type(b), f"{where}: {type(a).__name__} vs {type(b).__name__}"
    if isinstance(a, dict):
        assert list(a) == list(b), f"{where}: keys {list(a)} vs {list(b)}"
        for k in a:
            _same_struct(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), f"{where}: {len(a)} vs {len(b)} entries"
        for k, (x, y) in enumerate(zip(a, b)):
            _same_struct(x, y, f"{where}[{k}]")
    elif isinstance(a, (np.ndarray, np.generic, float)):
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{where}: {a} vs {b}"
    else:
        assert a == b, f"{where}: {a!r} vs {b!r}"


STEP_INFO_KEYS = ["game/shrine.wipes", "game/objects.wall", "attributes/steps", "attributes/seed", "agent/forged",
                  "agent/action.move.success", "agent/reward_step", "agent/reward_episode"]


def test_env_wrapper_with_every_reducer_on():
    """MettaGridBatchedEnv(specialize="sync") against specialize=False over 90 steps of 40-step episodes from a map pool (every
    env restarts on the device at least twice) with the episode statistics, the episode log, the per-step readout, the
    time-averaged stats, the per-policy stats, the token bag and the global state on."""
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    c = jc.case("torture")
    A = c.prog.num_agents
    pool = jc.class_maps(c, range(40, 47))
    kw = dict(map_pool=pool, pool_stride=3, seed=11, validate_actions=False, episode_stats=True, episode_log=64,
              step_info_keys=STEP_INFO_KEYS, time_averaged_stats=True, policy_assignments=[i % 2 for i in range(A)],
              token_bag=True, global_state=True)
    envs = [MettaGridBatchedEnv(c.prog, E, specialize=s, **kw) for s in ("sync", False)]
    try:
        for env in envs:
            env.reset()
        spec, plain = envs
        _assert_attached(spec.engine, "torture")
        assert plain.engine.obs_variant == 0 and plain.engine.handler_variant == 0

        def same(where):
            for env in envs:
                env.engine.sync()
            torch.cuda.synchronize()
            for k in ("obs", "rewards", "terminals", "truncations"):
                assert torch.equal(getattr(spec.engine, k), getattr(plain.engine, k)), f"{where}: '{k}'"
            for k, (x, y) in enumerate(zip(spec.token_bag + spec.global_state, plain.token_bag + plain.global_state)):
                assert torch.equal(x, y), f"{where}: token bag / global state tensor {k}"
            assert np.array_equal(spec.engine.state_digests(), plain.engine.state_digests()), f"{where}: digests"

        same("after reset")
        g = torch.Generator(device="cuda").manual_seed(5)
        aggregates, logs = [[], []], [[], []]
        for t in range(90):
            a = torch.randint(0, spec.transport_action_n, (E * A,), dtype=torch.int32, device="cuda", generator=g)
            outs = [env.step(a) for env in envs]
            same(f"step {t + 1}")
            for x, y in zip(outs[0][:4], outs[1][:4]):
                assert torch.equal(x, y), f"step {t + 1}: returned tensors"
            si = [o[4].pop("step_info") for o in outs]
            for k in ("game", "game_exists", "agent", "agent_exists"):
                assert torch.equal(getattr(si[0], k), getattr(si[1], k)), f"step {t + 1}: step_info.{k}"
            assert si[0].payload(32) == si[1].payload(32)
            for k in range(2):
                if outs[k][4]:
                    aggregates[k].append((t, outs[k][4]))
            if t % 30 == 29:
                for k in range(2):
                    logs[k] += envs[k].episode_infos()
        assert int(spec.engine.episodes()[0].min()) >= 2, "every env restarts on the device at least twice"
        assert len(logs[0]) >= 2 * E
        _same_struct(logs[0], logs[1], "episode_infos()")
        assert sum(i["episodes"] for _, i in aggregates[0]) >= 2 * E
        _same_struct(aggregates[0], aggregates[1], "aggregate infos")
        assert any("policy" in i for _, i in aggregates[0]) and any("time_averaged_game" in i for _, i in aggregates[0])
        assert spec.engine.poll_errors()[0] == 0 and plain.engine.poll_errors()[0] == 0
    finally:
        for env in envs:
            env.close()
