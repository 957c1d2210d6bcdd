"""Saving, loading and copying envs' state on the device (include/mgx.h mgx_save_envs / mgx_load_envs / mgx_copy_envs;
BatchedMettaGrid.save_envs / load_envs / copy_envs) against the oracle.

E = 70 envs, so that the env lists cross the 32-env wavefront and the 64-env workgroup boundaries.  A destination must
continue as an oracle of its source's (map, seed) that replays the source's actions up to the copy and the destination's
after it; every env nobody touched must still equal its own oracle."""
import numpy as np
import pytest

import helpers as hp
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import ENV_BAD_STATE, BatchedMettaGrid, EnvState, env_state_layout

pytestmark = pytest.mark.gpu

E = 70
FORKS = [(3, 64), (69, 0), (32, 31), (5, 10), (5, 11), (5, 40)]   # (source, destination): one source to several destinations


def _setup(name: str, n: int = E, buffers: str = "host", seeds=None):
    spec_f, map_f, _, invalid = hp.scenario(name)
    maps = [map_f(s) for s in range(n)]
    prog = hp.compile_scenario(name, spec_f(), *maps[0].shape)
    cms = np.stack([prog.class_map(m) for m in maps])
    seeds = np.arange(n, dtype=np.uint32) * 7 + 3 if seeds is None else seeds
    return prog, cms, seeds, BatchedMettaGrid(prog, cms, seeds, buffers=buffers), invalid


def _step(eng, acts, t):
    eng.actions[:] = np.concatenate([a[0][t] for a in acts])
    eng.vibe_actions[:] = np.concatenate([a[1][t] for a in acts])
    eng.step()


def _rows(snap, i, A):
    return {k: v[i * A:(i + 1) * A] for k, v in snap.items()}


def _outputs(eng):
    snap = eng.snapshot()
    return snap, eng.state_digests(), eng.current_steps()


def _payload_check(prog, eng, oracles, steps, seeds, where):
    A = prog.num_agents
    snap = eng.snapshot()
    for i, (o, seed) in oracles.items():
        pa = hp.payload_from_raw(prog, o.raw_objects(), o.current_stat_reward(), o.raw_stats(), o.snapshot(), steps, seed)
        pb = hp.payload_from_raw(prog, eng.raw_objects(i), eng.current_stat_reward(i), eng.raw_stats(i), _rows(snap, i, A), steps, seed)
        assert pa == pb, f"{where} env {i}: signature payload differs: {hp.diff_payload(pa, pb)}"


@pytest.mark.parametrize("name,k,m", [("rung3", 9, 8), ("rung4", 9, 8), ("dynamic", 9, 8), ("torture_terminal", 20, 8),
                                      ("rung4_truncating", 28, 7)])
def test_fork_against_oracle(name, k, m):
    import oracle_py as op
    prog, cms, seeds, eng, invalid = _setup(name)
    try:
        A = prog.num_agents
        acts = [hp.make_actions(prog, i, k + m, invalid) for i in range(E)]
        for t in range(k):
            _step(eng, acts, t)
        before = eng.state_digests()
        eng.copy_envs([s for s, _ in FORKS], [d for _, d in FORKS])
        after = eng.state_digests()   # (raises on MGX_ENV_INTERNAL)
        src_of = {d: s for s, d in FORKS}
        for i in range(E):
            assert after[i] == before[src_of.get(i, i)], f"{name}: digest of env {i} after the copy"
        oracles = {}
        for i in range(E):
            s = src_of.get(i, i)
            o = op.OracleSim(prog, cms[s], int(seeds[s]))
            o.reinit_buffers()
            for t in range(k):
                o.step(acts[s][0][t], acts[s][1][t])
            oracles[i] = (o, int(seeds[s]))
        snap = eng.snapshot()
        for i, (o, _) in oracles.items():
            hp.compare_snapshots(o.snapshot(), _rows(snap, i, A), f"{name} env {i} right after the copy")
        for t in range(k, k + m):
            _step(eng, acts, t)
            snap = eng.snapshot()
            for i, (o, _) in oracles.items():
                o.step(acts[i][0][t], acts[i][1][t])
                hp.compare_snapshots(o.snapshot(), _rows(snap, i, A), f"{name} env {i} step {t + 1}")
        bits, first = eng.poll_errors()
        assert bits == 0, f"{name}: env error bits {bits} (first env {first})"
        _payload_check(prog, eng, {i: oracles[i] for i in (0, 3, 10, 11, 31, 32, 40, 63, 64, 69)}, k + m, seeds, name)
    finally:
        eng.close()


@pytest.mark.parametrize("buffers", ["host", "device"])
@pytest.mark.parametrize("name", ["rung3", "dynamic"])
def test_save_step_load_step(name, buffers):
    prog, cms, seeds, eng, invalid = _setup(name, buffers=buffers)
    try:
        k, m = 4, 6
        acts = [hp.make_actions(prog, i, k + m, invalid) for i in range(E)]
        for t in range(k):
            _step(eng, acts, t) if buffers == "host" else _step_device(eng, acts, t)
        st = eng.save_envs()
        assert len(st) == E and st.envs.tolist() == list(range(E))
        first = []
        for t in range(k, k + m):
            _step(eng, acts, t) if buffers == "host" else _step_device(eng, acts, t)
            first.append(_outputs(eng) + (eng.episode_rewards(),))
        eng.load_envs(st)
        for j, t in enumerate(range(k, k + m)):
            _step(eng, acts, t) if buffers == "host" else _step_device(eng, acts, t)
            snap, dig, cur = _outputs(eng)
            hp.compare_snapshots(first[j][0], snap, f"{name} {buffers} step {t + 1} after the load")
            assert np.array_equal(first[j][1], dig) and np.array_equal(first[j][2], cur)
            assert np.array_equal(first[j][3], eng.episode_rewards())
        assert eng.poll_errors()[0] == 0
    finally:
        eng.close()


def _step_device(eng, acts, t):
    import torch
    eng.actions.copy_(torch.as_tensor(np.concatenate([a[0][t] for a in acts])))
    eng.vibe_actions.copy_(torch.as_tensor(np.concatenate([a[1][t] for a in acts])))
    eng.wait_for_caller()
    eng.step()
    eng.caller_waits()


def test_overlapping_copy_rotates():
    prog, cms, seeds, eng, invalid = _setup("rung3")
    try:
        A = prog.num_agents
        acts = [hp.make_actions(prog, i, 3, invalid) for i in range(E)]
        for t in range(3):
            _step(eng, acts, t)
        snap0, dig0, cur0 = _outputs(eng)
        eng.copy_envs([0, 1, 2], [1, 2, 0])
        snap1, dig1, cur1 = _outputs(eng)
        for s, d in ((0, 1), (1, 2), (2, 0)):
            assert dig1[d] == dig0[s]
            hp.compare_snapshots(_rows(snap0, s, A), _rows(snap1, d, A), f"rotation {s} -> {d}")
        assert np.array_equal(dig1[3:], dig0[3:])
        eng.copy_envs([0, 1], [1, 0])   # a swap
        assert np.array_equal(eng.state_digests()[:3], dig0[[0, 2, 1]])   # [d2, d0, d1] with 0 and 1 swapped
    finally:
        eng.close()


def test_pool_auto_reset_fork_against_oracle():
    """MettaGridBatchedEnv with a map pool, lazy auto-reset, the early-reset desync and episode statistics.  One env is forked
    on the step its episode ends: the destination restarts next step on ITS slot's pool map and seed.  Another is forked
    inside its first (early-ending) episode and then given the source's actions: the two episodes' records agree apart from
    the env index and the slot's seed."""
    import oracle_py as op
    from mettagrid_amd.envs import MettaGridBatchedEnv
    M, stride, n, max_steps = 7, 3, 6, 11
    spec = presets.rung2_spec()
    spec.max_steps = max_steps
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    pool = np.stack([prog.class_map(presets.rung2_map(50 + m)) for m in range(M)])
    env = MettaGridBatchedEnv(prog, n, map_pool=pool, pool_stride=stride, desync=True, seed=7, buffers="host",
                              episode_stats=True, episode_log=256)
    env.reset()
    try:
        A = prog.num_agents
        early = [int(x) for x in env.early_end_steps()]
        seeds = [(7 + e) & 0xFFFFFFFF for e in range(n)]
        episode = [0] * n
        hist = [(pool[e % M], seeds[e], []) for e in range(n)]   # (map, seed, actions) of every env's current episode
        oracles = [op.OracleSim(prog, pool[e % M], seeds[e]) for e in range(n)]
        for o in oracles:
            o.reinit_buffers()
        ended = [False] * n
        rng = np.random.default_rng(5)
        n_primary = len(env.action_names)
        forked_end = forked_mid = None
        follow = {}   # destination -> source whose actions it receives

        def expected(e):   # the oracle's rows + the early end of a first episode, which truncates every agent of the env
            s = dict(oracles[e].snapshot())
            if episode[e] == 0 and oracles[e].current_step >= early[e]:
                s["truncations"] = np.ones_like(s["truncations"])
            return s
        for t in range(40):
            for e in range(n):
                if ended[e]:
                    episode[e] += 1
                    mp = pool[(e + episode[e] * stride) % M]
                    oracles[e] = op.OracleSim(prog, mp, seeds[e])
                    oracles[e].reinit_buffers()
                    hist[e] = (mp, seeds[e], [])
                    ended[e] = False
                    follow.pop(e, None)
            a = rng.integers(0, n_primary, size=n * A).astype(np.int32)
            for d, s in follow.items():
                a[d * A:(d + 1) * A] = a[s * A:(s + 1) * A]
            env.step(a)
            for e, o in enumerate(oracles):
                o.step(a[e * A:(e + 1) * A], np.zeros(A, np.int32))
                hist[e][2].append(a[e * A:(e + 1) * A].copy())
            snap = env.engine.snapshot()
            for e in range(n):
                hp.compare_snapshots(expected(e), _rows(snap, e, A), f"pool env {e} step {t + 1}")
            for e, o in enumerate(oracles):
                s = o.snapshot()
                ended[e] = bool(s["truncations"].all() or s["terminals"].all() or (episode[e] == 0 and o.current_step >= early[e]))

            def fork(s, d):
                env.engine.copy_envs([s], [d])
                mp, sd, hs = hist[s]
                o = op.OracleSim(prog, mp, sd)
                o.reinit_buffers()
                for x in hs:
                    o.step(x, np.zeros(A, np.int32))
                oracles[d], hist[d] = o, (mp, sd, [x.copy() for x in hs])
                episode[d], ended[d], early[d] = episode[s], ended[s], early[s]
                hp.compare_snapshots(expected(d), _rows(env.engine.snapshot(), d, A), f"pool fork {s} -> {d} step {t + 1}")

            if forked_end is None and t >= 2:
                done = [e for e in range(n) if ended[e]]
                if done:
                    s = done[0]
                    d = next(e for e in range(n) if e != s and not ended[e] and e not in follow and e not in follow.values())
                    fork(s, d)
                    forked_end = (s, d, episode[s])
            if forked_mid is None and t >= 1:
                cand = [e for e in range(n) if episode[e] == 0 and not ended[e] and early[e] > t + 3]
                if len(cand) >= 2:
                    s, d = cand[0], cand[1]
                    fork(s, d)
                    follow[d] = s
                    forked_mid = (s, d)
        assert forked_end is not None and forked_mid is not None
        s, d, ep = forked_end
        eps, mi = env.engine.episodes()
        assert eps.tolist() == episode and mi.tolist() == [(e + episode[e] * stride) % M for e in range(n)]
        recs = env.engine.drain_episode_log()[0]
        s, d = forked_mid
        rs = [r for r in recs if r["env"] == s and r["episode"] == 0]
        rd = [r for r in recs if r["env"] == d and r["episode"] == 0]
        assert len(rs) == 1 and len(rd) == 1, (len(rs), len(rd))
        a, b = dict(rs[0]), dict(rd[0])
        for key in ("env", "seed"):
            a.pop(key), b.pop(key)
        assert repr(a) == repr(b)
        assert env.engine.poll_errors()[0] == 0
    finally:
        env.close()


def test_across_engines(tmp_path):
    prog, cms, seeds, a, invalid = _setup("rung4")
    try:
        A = prog.num_agents
        acts = [hp.make_actions(prog, i, 10, invalid) for i in range(E)]
        for t in range(5):
            _step(a, acts, t)
        assert a.env_state_info() == env_state_layout(prog, cms)
        st = a.save_envs([7, 66])
        np.savez(tmp_path / "state.npz", **st.to_dict())
        # engine B: 5 envs whose create maps include A's maps of envs 7 and 66 (the same capacities)
        cms_b = np.stack([cms[66], cms[1], cms[2], cms[3], cms[7]])
        b = BatchedMettaGrid(prog, cms_b, np.arange(5, dtype=np.uint32) + 100, buffers="host")
        try:
            assert b.env_state_info() == env_state_layout(prog, cms_b)
            assert b.env_state_info()["format"] == a.env_state_info()["format"]
            b.load_envs(EnvState.from_dict(np.load(tmp_path / "state.npz")), [4, 0])
            for t in range(5, 10):
                _step(a, acts, t)
                b.actions[:] = np.concatenate([acts[66][0][t], acts[1][0][t], acts[2][0][t], acts[3][0][t], acts[7][0][t]])
                b.vibe_actions[:] = np.concatenate([acts[66][1][t], acts[1][1][t], acts[2][1][t], acts[3][1][t], acts[7][1][t]])
                b.step()
                sa, sb = a.snapshot(), b.snapshot()
                hp.compare_snapshots(_rows(sa, 7, A), _rows(sb, 4, A), f"A env 7 / B env 4 step {t + 1}")
                hp.compare_snapshots(_rows(sa, 66, A), _rows(sb, 0, A), f"A env 66 / B env 0 step {t + 1}")
            da, db = a.state_digests(), b.state_digests()
            assert da[7] == db[4] and da[66] == db[0]
        finally:
            b.close()
    finally:
        a.close()


def _unchanged(eng):
    snap, dig, cur = _outputs(eng)
    return lambda where: (hp.compare_snapshots(snap, eng.snapshot(), where),
                          np.testing.assert_array_equal(dig, eng.state_digests(), where),
                          np.testing.assert_array_equal(cur, eng.current_steps(), where))


def test_refusals_leave_everything_unchanged(monkeypatch):
    prog, cms, seeds, eng, invalid = _setup("rung4", n=8)
    try:
        acts = [hp.make_actions(prog, i, 3, invalid) for i in range(8)]
        for t in range(3):
            _step(eng, acts, t)
        st = eng.save_envs([1, 2])
        same = _unchanged(eng)
        # another program
        p3, c3, s3, other, _ = _setup("rung3", n=2)
        try:
            with pytest.raises(ValueError, match="format"):
                other.load_envs(st, [0, 1])
        finally:
            other.close()
        # the same program created with maps that set other AoE / territory capacities
        few = np.stack([prog.class_map(hp.random_map(20, 22, {"wall": 18, "healer": 1, "fire": 1, "hub": 2, "wire": 10, "flag_red": 1},
                                                     {"red": 4, "blue": 4, "green": 4}, s)) for s in range(2)])
        thin = BatchedMettaGrid(prog, few, [1, 2], buffers="host")
        try:
            u = _unchanged(thin)
            with pytest.raises(ValueError, match="format"):
                thin.load_envs(st, [0, 1])
            u("other capacities")
        finally:
            thin.close()
        # integer bookkeeping is part of the format
        monkeypatch.setenv("MGX_NO_SHADOW", "1")
        p4, c4, s4, ns, _ = _setup("rung3", n=2)
        monkeypatch.delenv("MGX_NO_SHADOW")
        p5, c5, s5, sh, _ = _setup("rung3", n=2)
        try:
            assert ns.paths["shadow"] is False and sh.paths["shadow"] is True
            u = _unchanged(ns)
            with pytest.raises(ValueError, match="format"):
                ns.load_envs(sh.save_envs([0, 1]), [0, 1])
            u("MGX_NO_SHADOW")
        finally:
            ns.close()
            sh.close()
        for bad in ([1, 1], [0, 8], []):
            with pytest.raises(ValueError):
                eng.load_envs(st, bad)
            with pytest.raises(ValueError):
                eng.copy_envs([0, 1][:len(bad)], bad)
        # the C entry points refuse on their own (the Python checks bypassed)
        import ctypes
        info = st.info_struct()
        for bad in ([1, 1], [0, 8], [-1, 0]):
            lst = np.asarray(bad, np.int32)
            assert eng.L.mgx_load_envs(eng.h, lst.ctypes.data, 2, ctypes.c_void_p(st.data.ctypes.data), ctypes.byref(info)) == -1
        assert eng.L.mgx_load_envs(eng.h, np.zeros(1, np.int32).ctypes.data, 0, ctypes.c_void_p(st.data.ctypes.data), ctypes.byref(info)) == -1
        same("refused loads")
    finally:
        eng.close()


def test_box_output_refused():
    import torch
    prog, cms, seeds, eng, invalid = _setup("rung3", n=4, buffers="device")
    try:
        st = eng.save_envs([0])
        from mettagrid_amd.fmt import K
        H, W = int(prog.words[K.H_OBS_HEIGHT]), int(prog.words[K.H_OBS_WIDTH])
        box = torch.zeros((4 * prog.num_agents, len(prog.feature_norms), H, W), dtype=torch.float32, device="cuda")
        eng.set_box_output(box)
        same = _unchanged(eng)
        with pytest.raises(ValueError, match="box"):
            eng.load_envs(st, [1])
        import ctypes
        info = st.info_struct()
        lst = np.asarray([1], np.int32)
        assert eng.L.mgx_load_envs(eng.h, lst.ctypes.data, 1, ctypes.c_void_p(st.data.data_ptr()), ctypes.byref(info)) == -1
        same("box output on")
    finally:
        eng.close()


@pytest.mark.parametrize("switch", ["MGX_NO_DUO", "MGX_OBS_GENERIC"])
def test_speed_paths_load_the_state(switch, monkeypatch):
    import oracle_py as op
    prog, cms, seeds, eng, invalid = _setup("rung3", n=4)
    try:
        A = prog.num_agents
        acts = [hp.make_actions(prog, i, 8, invalid) for i in range(4)]
        for t in range(4):
            _step(eng, acts, t)
        st = eng.save_envs()
        monkeypatch.setenv(switch, "1")
        _, _, _, other, _ = _setup("rung3", n=4)
        try:
            assert other.paths != eng.paths or switch == "MGX_OBS_GENERIC"
            assert other.env_state_info()["format"] == eng.env_state_info()["format"]
            other.load_envs(st)
            oracles = []
            for i in range(4):
                o = op.OracleSim(prog, cms[i], int(seeds[i]))
                o.reinit_buffers()
                for t in range(4):
                    o.step(acts[i][0][t], acts[i][1][t])
                oracles.append(o)
            for t in range(4, 8):
                _step(other, acts, t)
                snap = other.snapshot()
                for i, o in enumerate(oracles):
                    o.step(acts[i][0][t], acts[i][1][t])
                    hp.compare_snapshots(o.snapshot(), _rows(snap, i, A), f"{switch} env {i} step {t + 1}")
        finally:
            other.close()
    finally:
        eng.close()


def test_bad_record_sets_the_error_bit_of_that_env_only():
    prog, cms, seeds, eng, invalid = _setup("rung3", n=8)
    try:
        acts = [hp.make_actions(prog, i, 2, invalid) for i in range(8)]
        for t in range(2):
            _step(eng, acts, t)
        st = eng.save_envs([2, 3, 4])
        dig = eng.state_digests()
        st.data[1, 8] ^= 0xFF   # record 1's format word: another layout
        eng.load_envs(st, [5, 6, 7])
        bits, first = eng.poll_errors()
        assert bits == ENV_BAD_STATE and first == 6
        new = eng.state_digests()
        assert new[5] == dig[2] and new[7] == dig[4] and new[6] == dig[6]
    finally:
        eng.close()


def test_full_size_rung3():
    import oracle_py as op
    n = 65536
    maps = [presets.rung3_map(s) for s in range(4)]
    prog = compile_spec(presets.rung3_spec(), *maps[0].shape)
    cms = np.stack([prog.class_map(maps[i % 4]) for i in range(n)])
    seeds = np.arange(n, dtype=np.uint32) * 7 + 3
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="device", specialize=False)
    try:
        A = prog.num_agents
        rng = np.random.default_rng(1)
        acts = [rng.integers(0, len(prog.action_names), size=n * A).astype(np.int32) for _ in range(9)]

        def step(t):
            import torch
            eng.actions.copy_(torch.as_tensor(acts[t]))
            eng.vibe_actions.zero_()
            eng.wait_for_caller()
            eng.step()
            eng.caller_waits()

        st = eng.save_envs()
        first = []
        for t in range(3):
            step(t)
            first.append(eng.state_digests())
        eng.load_envs(st)
        for t in range(3):
            step(t)
            assert np.array_equal(first[t], eng.state_digests()), f"step {t + 1} after the load"
        half = n // 2
        eng.copy_envs(np.arange(half), np.arange(half, n))
        dig = eng.state_digests()
        assert np.array_equal(dig[:half], dig[half:])
        sample = (0, 31, 32, 63, 64, 32767, 65535)
        oracles = {}
        for i in sample:
            s = i % half
            o = op.OracleSim(prog, cms[s], int(seeds[s]))
            o.reinit_buffers()
            for t in range(3):
                o.step(acts[t][s * A:(s + 1) * A], np.zeros(A, np.int32))
            oracles[i] = o
        for t in range(3, 6):
            step(t)
            snap = eng.snapshot()
            for i, o in oracles.items():
                o.step(acts[t][i * A:(i + 1) * A], np.zeros(A, np.int32))
                hp.compare_snapshots(o.snapshot(), _rows(snap, i, A), f"full size env {i} step {t + 1}")
        assert eng.poll_errors()[0] == 0
    finally:
        eng.close()
