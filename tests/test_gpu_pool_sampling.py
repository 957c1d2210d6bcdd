"""GPU: weighted draws of the next pool map at auto-reset and per-map episode statistics (include/mgx.h "Weighted map-pool
sampling"; csrc/mgx_pool_sample.h).  The draw is numpy's own stream keyed by (env, episode) and the table is integer, so every
comparison is exact: against the numpy restatement (mettagrid_amd/pool_sampling.py, pinned to numpy's generator by
tests/test_pool_sampling_host.py), against an oracle mirror of every env, and against the episode log."""
import numpy as np
import pytest

import oracle_py as op
from mettagrid_amd import engine as engine_mod
from mettagrid_amd import pool_sampling as ps
from mettagrid_amd.early_reset import first_integers
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv
from test_gpu_time_avg import _program, _random_actions

pytestmark = pytest.mark.gpu

E, M, STRIDE = 70, 5, 3            # a full wavefront plus a remainder
W = [3, 0, 1, 0.5, 1e-12]          # a zero weight, and a positive one whose interval is one word wide
SEED = 4242
MAX_STEPS = 5


@pytest.fixture(scope="module")
def game():
    prog, pool = _program("rung3", MAX_STEPS)
    return prog, np.ascontiguousarray(pool[:M])


def _seeds(n):
    return (11 + np.arange(n)).astype(np.uint32)


def _engine(prog, pool, n=E, desync=True, weights=W, offset=0, ep_stats=True, ms=False, log=None):
    early = first_integers(_seeds(n), MAX_STEPS) if desync else None
    eng = BatchedMettaGrid(prog, pool[np.arange(n) % M], _seeds(n), buffers="host")
    eng.set_map_pool(pool)
    eng.set_auto_reset(True, STRIDE, early)
    if ep_stats:
        eng.set_episode_stats(True, log_capacity=log or 8 * n)
    if weights is not None:
        eng.set_pool_sampling(weights, SEED, offset)
    if ms:
        eng.set_map_stats(True)
    return eng, early


def _step(eng, prog, rng, n=E):
    a, v = _random_actions(rng, prog, n)
    eng.actions[:] = a
    eng.vibe_actions[:] = v
    eng.step()
    return a, v


def _want(envs, episodes, weights=W, offset=0):
    return ps.draws(weights, SEED, offset, envs, episodes)


@pytest.mark.parametrize("offset", [0, 2**32 - 3])
def test_pool_draws_equal_the_restatement(game, offset):
    """70 envs x 9 episodes plus the corner keys; offset 2**32 - 3: the stream key a = (offset + env) mod 2**32 wraps."""
    prog, pool = game
    eng, _ = _engine(prog, pool, offset=offset, ep_stats=False)
    envs, eps = (x.reshape(-1) for x in np.meshgrid(np.arange(E), np.arange(1, 10), indexing="ij"))
    envs = np.concatenate([envs, [0, 0, E - 1, E - 1, 2, 3]])
    eps = np.concatenate([eps, [0, 2**32 - 1, 0, 2**32 - 1, 2**31, 2**31 - 1]]).astype(np.uint64)
    got = eng.pool_draws(envs, eps)
    want = _want(envs, eps, offset=offset)
    assert np.array_equal(got, want)
    # ... and numpy's own generator, on a sample
    edges = ps.quantise(W)
    for i in range(0, len(envs), 41):
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(SEED, spawn_key=((offset + int(envs[i])) % 2**32, int(eps[i])))))
        assert got[i] == np.searchsorted(edges, int(g.integers(0, 2**32, dtype=np.uint32)), side="right")
    assert set(np.unique(got)) <= {0, 2, 3} and len(np.unique(got)) == 3
    assert eng.pool_draws([], []).size == 0
    with pytest.raises(ValueError):
        eng.pool_draws([E], [1])
    eng.close()


class Mirror:
    """One oracle env per engine env, restarted as the engine's lazy auto-reset restarts it; ``index(env, episode)`` names the
    pool map of episodes > 0 (the first plays env mod M).  The mirror of tests/test_gpu_time_avg.py with the rotation rule
    replaced."""

    def __init__(self, prog, pool, seeds, early, index):
        self.prog, self.pool, self.seeds, self.early, self.index = prog, pool, seeds, early, index
        self.E, self.A = len(seeds), prog.num_agents
        self.episode, self.ended = [0] * self.E, [False] * self.E
        self.map_index = [e % len(pool) for e in range(self.E)]
        self.oracles = [self._new(e) for e in range(self.E)]

    def _new(self, e):
        if self.episode[e] > 0:
            self.map_index[e] = int(self.index(e, self.episode[e]))
        o = op.OracleSim(self.prog, self.pool[self.map_index[e]], int(self.seeds[e]))
        o.reinit_buffers()
        return o

    def step(self, a, v):
        """-> obs, rewards, terminals, truncations of the whole batch after the step (early ends marked as truncations)."""
        A, out = self.A, {"obs": [], "rewards": [], "terminals": [], "truncations": []}
        for e in range(self.E):
            if self.ended[e]:
                self.episode[e] += 1
                self.oracles[e], self.ended[e] = self._new(e), False
            o = self.oracles[e]
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            s = o.snapshot()
            early_end = self.early is not None and self.episode[e] == 0 and o.current_step >= self.early[e] > 0
            trunc = np.ones_like(s["truncations"]) if early_end else s["truncations"]
            self.ended[e] = bool(s["terminals"].all()) or bool(trunc.all())
            for k, x in (("obs", s["obs"]), ("rewards", s["rewards"]), ("terminals", s["terminals"]), ("truncations", trunc)):
                out[k].append(x)
        return {k: np.concatenate(x) for k, x in out.items()}


def test_auto_reset_plays_the_drawn_maps_against_oracle(game):
    """40 steps of 5-step episodes with desync: after every step the engine's indices are the restatement's and observations,
    rewards and done flags are those of oracle envs built from the drawn maps."""
    prog, pool = game
    eng, early = _engine(prog, pool, ep_stats=False)
    mirror = Mirror(prog, pool, _seeds(E), early, lambda e, k: _want([e], [k])[0])
    rng = np.random.default_rng(5)
    played = set()
    for t in range(40):
        a, v = _step(eng, prog, rng)
        m = mirror.step(a, v)
        ep, mi = eng.episodes()
        assert np.array_equal(ep, mirror.episode), t
        live = ep > 0
        assert np.array_equal(mi[live], _want(np.nonzero(live)[0], ep[live])), t
        assert np.array_equal(mi[live], np.asarray(mirror.map_index)[live]), t   # (a first episode has no pool index)
        played |= set(mi[live].tolist())
        assert np.array_equal(eng.obs, m["obs"]), t
        assert np.array_equal(eng.rewards, m["rewards"]), t
        assert np.array_equal(np.asarray(eng.terminals, bool), m["terminals"].astype(bool)), t
        assert np.array_equal(np.asarray(eng.truncations, bool), m["truncations"].astype(bool)), t
    assert played == {0, 2, 3} and int(ep.min()) >= 6   # maps 1 and 4 are never played
    assert eng.poll_errors()[0] & ~2 == 0
    eng.close()


def test_set_pool_weights_and_off(game):
    """One-hot weights between two steps: every restart from the next step on plays that map and running episodes keep theirs;
    of two calls without a step between them the last wins; sampling off: the rotation rule's indices again."""
    prog, pool = game
    eng, _ = _engine(prog, pool, ep_stats=False)
    rng = np.random.default_rng(6)
    for t in range(9):
        _step(eng, prog, rng)
    ep0, mi0 = eng.episodes()
    assert np.array_equal(mi0[ep0 > 0], _want(np.nonzero(ep0 > 0)[0], ep0[ep0 > 0]))
    eng.set_pool_weights([0, 1, 0, 0, 0])
    eng.set_pool_weights([0, 0, 0, 0, 2.5])       # the last wins
    assert np.array_equal(eng.pool_draws(np.arange(E), np.full(E, 3)), np.full(E, 4))
    for t in range(7):
        _step(eng, prog, rng)
        ep, mi = eng.episodes()
        same = ep == ep0
        assert np.array_equal(mi[same], mi0[same]) and (mi[~same] == 4).all(), t
    assert (ep > ep0).all()
    eng.set_pool_sampling(None)
    ep1, mi1 = eng.episodes()
    for t in range(7):
        _step(eng, prog, rng)
        ep, mi = eng.episodes()
        same = ep == ep1
        assert np.array_equal(mi[same], mi1[same]), t
        assert np.array_equal(mi[~same], ((np.arange(E) + ep.astype(np.int64) * STRIDE) % M)[~same]), t
    assert (ep > ep1).all()
    with pytest.raises(ValueError, match="sampling is off"):
        eng.set_pool_weights(W)
    eng.close()


def _host_table(recs, A):
    return ps.MapStatsHost(M, A).add(recs).table


def test_map_stats_equal_the_log_window_by_window(game):
    """Nothing dropped from the log: every snapshot window's table equals MapStatsHost over the same window's records, word for
    word; the unattributed row counts the window's first episodes; a window without episodes is the cleared table."""
    prog, pool = game
    eng, _ = _engine(prog, pool, ms=True)
    rng = np.random.default_rng(7)
    cleared = np.tile(ps.MS_EMPTY, (M + 1, 1))
    eng.request_map_stats()                        # nothing has finished yet
    assert np.array_equal(eng.fetch_map_stats(wait=True, raw=True), cleared)
    assert eng.fetch_map_stats(wait=True) is None  # fetched: no snapshot is pending
    n_first = n_all = 0
    for t in range(42):
        _step(eng, prog, rng)
        if (t + 1) % 7 == 0:
            if t % 2:
                got = eng.drain_map_stats(raw=True)
            else:
                eng.request_map_stats()
                eng.request_map_stats()            # (a second request while one is pending changes nothing)
                got = eng.fetch_map_stats(wait=True, raw=True)
            recs, dropped = eng.drain_episode_log()
            assert dropped == 0 and len(recs) > 0
            want = _host_table(recs, prog.num_agents)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (t, got, want)
            first = sum(r["episode"] == 0 for r in recs)
            assert int(got[M, 0]) == first == sum(r["map_index"] == -1 for r in recs)
            assert int(got[:, 0].sum()) == len(recs) and got[1, 0] == 0 and got[4, 0] == 0
            n_first += first
            n_all += len(recs)
            assert np.array_equal(eng.drain_map_stats(raw=True), cleared)   # no step in between: no finished episode
    assert n_first == E and n_all >= 7 * E
    d = eng.drain_map_stats()
    assert len(d) == M + 1 and set(d[0]) == {"episodes", "terminated", "length_sum", "return_sum", "return_min", "return_max"}
    eng.set_episode_stats(True, log_capacity=16)   # setting the episode statistics again switches the table off
    with pytest.raises(ValueError, match="map statistics are off"):
        eng.request_map_stats()
    eng.close()


def test_map_stats_when_every_env_finishes_at_once(game):
    """300 envs without desync: all finish in one step — first 300 adds to the unattributed row, then 300 spread over three
    rows — and the table is still exact."""
    prog, pool = game
    n = 300
    eng, _ = _engine(prog, pool, n=n, desync=False, ms=True, log=2 * n)
    rng = np.random.default_rng(8)
    for rnd in range(2):
        for t in range(MAX_STEPS):
            _step(eng, prog, rng, n)
        got = eng.drain_map_stats(raw=True)
        recs, dropped = eng.drain_episode_log()
        assert dropped == 0 and len(recs) == n and all(r["episode"] == rnd for r in recs)
        assert np.array_equal(got, _host_table(recs, prog.num_agents)), rnd
        assert int(got[M, 0]) == (n if rnd == 0 else 0)
    assert (got[[0, 2, 3], 0] > 0).all()
    eng.close()


def test_forked_env_draws_with_its_own_slot(game):
    """copy_envs(3 -> 68) mid-run: env 68's next map is the restatement's for slot 68 and the moved episode count + 1; the
    saved record is as large as without sampling."""
    prog, pool = game
    eng, _ = _engine(prog, pool, weights=None, ep_stats=False)
    bytes_before = eng.env_state_info()["record_bytes"]
    eng.set_pool_sampling(W, SEED, 0)
    assert eng.env_state_info()["record_bytes"] == bytes_before
    rng = np.random.default_rng(9)
    for t in range(13):
        _step(eng, prog, rng)
    ep, mi = eng.episodes()
    eng.copy_envs([3], [68])
    ep2, mi2 = eng.episodes()
    assert ep2[68] == ep[3] and mi2[68] == mi[3]
    moved = int(ep[3])
    for t in range(MAX_STEPS + 1):
        _step(eng, prog, rng)
        ep3, mi3 = eng.episodes()
        if ep3[68] > moved:
            break
    assert ep3[68] == moved + 1
    assert mi3[68] == _want([68], [moved + 1])[0]
    live = ep3 > 0
    assert np.array_equal(mi3[live], _want(np.nonzero(live)[0], ep3[live]))
    assert eng.env_state_info()["record_bytes"] == bytes_before == engine_mod.env_state_layout(prog, pool)["record_bytes"]
    eng.close()


def test_refusals_leave_the_earlier_setting(game):
    prog, pool = game
    L = engine_mod.load_lib()
    # no pool
    bare = BatchedMettaGrid(prog, pool[np.arange(4) % M], _seeds(4), buffers="host")
    with pytest.raises(ValueError, match="no map pool"):
        bare.set_pool_sampling(W, SEED)
    w = np.array(W, np.float64)
    assert L.mgx_set_pool_sampling(bare.h, w.ctypes.data, 1, 0) == -1 and b"no map pool" in L.mgx_last_error()
    bare.set_episode_stats(True)
    with pytest.raises(ValueError, match="no map pool"):
        bare.set_map_stats(True)
    bare.close()
    eng, _ = _engine(prog, pool, ep_stats=False)
    probe = (np.arange(E), np.arange(E) % 9 + 1)
    before = eng.pool_draws(*probe)
    assert np.array_equal(before, _want(*probe))
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5, 6]):                      # a wrong weight count
        with pytest.raises(ValueError, match="shape"):
            eng.set_pool_sampling(bad, SEED + 1)
        with pytest.raises(ValueError, match="shape"):
            eng.set_pool_weights(bad)
    for bad in ([1, -1, 1, 1, 1], [1, float("nan"), 1, 1, 1], [1, float("inf"), 1, 1, 1], [0, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match="weight"):
            eng.set_pool_sampling(bad, SEED + 1)
        with pytest.raises(ValueError, match="weight"):
            eng.set_pool_weights(bad)
    assert np.array_equal(eng.pool_draws(*probe), before)             # seed and thresholds as before
    with pytest.raises(ValueError, match="episode statistics are off"):
        eng.set_map_stats(True)                                       # map stats without episode stats
    with pytest.raises(ValueError, match="pool sampling"):
        eng.set_map_pool(pool[:3])                                    # a pool of another size while sampling is on
    eng.set_map_pool(pool[::-1].copy())                               # the same size keeps it
    assert np.array_equal(eng.pool_draws(*probe), before)
    eng.set_pool_sampling(None)
    eng.set_episode_stats(True)
    eng.set_map_stats(True)
    with pytest.raises(ValueError, match="map statistics"):
        eng.set_map_pool(pool[:3])                                    # ... or while the table is on
    eng.set_map_stats(False)
    eng.set_map_pool(pool[:3])
    with pytest.raises(ValueError, match="sampling is off"):
        eng.pool_draws([0], [1])
    eng.close()


def _f64_return_sum(rewards) -> float:
    s = 0.0
    for x in rewards:   # the record's sum: the agents' f32 episode rewards added in agent order as f64
        s += float(x)
    return s


def test_wrapper_infos(game):
    """MettaGridBatchedEnv(map_weights=..., map_stats=True, map_labels=...) on device buffers: every non-empty infos carries the
    table of exactly its window's episodes (taken from episode_infos() in log order) and the per-label mean returns;
    set_map_weights redirects the restarts; without the arguments infos has today's keys."""
    import torch
    prog, pool = game
    A = prog.num_agents
    labels = ["easy", "never", "easy", "hard", "never"]
    kw = dict(map_pool=pool, pool_stride=STRIDE, seed=11, validate_actions=False, desync=True, episode_log=2048, stats_interval=3)
    env = MettaGridBatchedEnv(prog, E, map_weights=W, map_sample_seed=SEED, map_stats=True, map_labels=labels, **kw)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    windows = []
    for t in range(36):
        if t == 24:
            env.set_map_weights([0, 0, 0, 1, 0])
        a = torch.randint(0, env.transport_action_n, (E * A,), device="cuda", dtype=torch.int32, generator=g)
        *_, infos = env.step(a)
        env.engine.sync()   # (so that the snapshot requested one interval ago has landed: the wrapper itself never waits)
        if infos:
            windows.append(infos)
    env.engine.sync()
    entries = env.episode_infos()
    assert env.episodes_dropped == 0 and len(windows) >= 4
    ep, mi = env.engine.episodes()
    assert (mi == 3).all()   # 12 steps after set_map_weights every env has restarted (episodes last at most 5 steps)
    late = [i for i in entries if i["episode"] > 0]
    # episode k of an env starts no later than step 5 k: up to k = 4 the first weights drew it
    early_ones = [i for i in late if i["episode"] <= 4]
    assert len(early_ones) >= 3 * E
    assert np.array_equal([i["map_index"] for i in early_ones], _want([i["env"] for i in early_ones], [i["episode"] for i in early_ones]))
    assert all(i["map_index"] in (0, 2, 3) for i in late) and all(i["map_index"] == -1 for i in entries if i["episode"] == 0)
    k = 0
    for infos in windows:
        n = infos["episodes"]
        recs = [{"map_index": i["map_index"], "steps": i["attributes"]["steps"], "flags": 0, "return_sum": _f64_return_sum(i["episode_rewards"])}
                for i in entries[k:k + n]]
        k += n
        want = ps.table_dicts(_host_table(recs, A))
        got = infos["per_map"] + [infos["unattributed"]]
        assert len(infos["per_map"]) == M
        for x, y in zip(got, want):
            y = dict(y, terminated=x["terminated"])   # (episode_infos() entries do not carry the flags; the engine test compares them)
            assert x == y, (x, y)
        tot = {}
        for label, m in zip(labels, want):
            if m["episodes"]:
                t = tot.setdefault(label, [0.0, 0])
                t[0] += m["return_sum"]
                t[1] += m["episodes"]
        assert infos["per_label_rewards"] == {label: t[0] / t[1] for label, t in tot.items()}
        assert "never" not in infos["per_label_rewards"]
    assert k <= len(entries)
    rest = env.engine.drain_map_stats()
    assert k + sum(m["episodes"] for m in rest) == len(entries)
    env.close()
    plain = MettaGridBatchedEnv(prog, 6, **kw)
    plain.reset()
    keys = set()
    for t in range(12):
        a = torch.zeros(6 * A, device="cuda", dtype=torch.int32)
        *_, infos = plain.step(a)
        keys |= set(infos)
    assert keys == {"episodes", "game", "agent", "game_count", "agent_count", "episode_return", "episode_length", "terminated", "attributes"}
    with pytest.raises(ValueError, match="no map_weights"):
        plain.set_map_weights(W)
    plain.close()
    uni = MettaGridBatchedEnv(prog, 6, map_weights="uniform", **kw)
    assert uni.map_weights.tolist() == [1.0] * M
    for bad in (dict(map_weights=W, map_fn=lambda e, k: pool[0], map_pool=None), dict(map_stats=True, episode_stats=False),
                dict(map_weights=[1, 2]), dict(map_weights=[1, -1, 1, 1, 1]), dict(map_labels=labels)):
        with pytest.raises(ValueError):
            MettaGridBatchedEnv(prog, 6, **dict(kw, **bad))
