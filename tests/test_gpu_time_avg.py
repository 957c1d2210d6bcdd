"""GPU: time-averaged game stats of every episode, accumulated on the device (include/mgx.h "Time-averaged game stats";
the reference's TimeAveragedStatsHandler, python/src/mettagrid/simulator/time_averaged_stats.py:17-41).  Every env is mirrored
by an oracle env under the suite's restatement of the handler (tests/test_time_avg_fixture.py, pinned there to the reference's
own handler); key sets and f64 values are compared bit for bit, the batch totals with the same sums taken on the host in the
engine's documented order."""
import numpy as np
import pytest

import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.early_reset import first_integers
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv
from mettagrid_amd.summary import summarize_episodes
from test_time_avg_fixture import TimeAveragedStats, oracle_game, same_f64_dict

pytestmark = pytest.mark.gpu

M, STRIDE = 7, 3


def _program(workload: str, max_steps: int):
    if workload == "rung4":
        prog = compile_spec(presets.rung4_spec(max_steps=max_steps), 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
        return prog, np.stack([prog.class_map(presets.rung4_map(50 + m)) for m in range(M)])
    spec = presets.rung2_spec() if workload == "rung2" else presets.rung3_spec()
    spec.max_steps = max_steps
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    mk = presets.rung2_map if workload == "rung2" else presets.rung3_map
    return prog, np.stack([prog.class_map(mk(50 + m)) for m in range(M)])


def _engine(prog, pool, E, early, log=None, ta=True, stride=STRIDE):
    seeds = (11 + np.arange(E)).astype(np.uint32)
    eng = BatchedMettaGrid(prog, pool[np.arange(E) % M], seeds, buffers="host")
    eng.set_map_pool(pool)
    eng.set_auto_reset(True, stride, early)
    log = 5 * E if log is None else log
    eng.set_episode_stats(True, log_capacity=log)
    if ta:
        eng.set_time_averages(True, log_capacity=log)
    return eng, seeds


class Mirror:
    """One oracle env + one handler per engine env, restarted when the engine's auto-reset restarts it."""

    def __init__(self, prog, pool, seeds, early, stride=STRIDE):
        self.prog, self.pool, self.seeds, self.early, self.stride = prog, pool, seeds, early, stride
        self.E, self.A = len(seeds), prog.num_agents
        self.episode, self.ended = [0] * self.E, [False] * self.E
        self.oracles = [self._new(e) for e in range(self.E)]
        self.handlers = [TimeAveragedStats() for _ in range(self.E)]

    def _new(self, e):
        o = op.OracleSim(self.prog, self.pool[(e + self.episode[e] * self.stride) % len(self.pool)], int(self.seeds[e]))
        o.reinit_buffers()
        return o

    def step(self, a, v) -> list:
        """-> this step's finished episodes in ascending env index: {env, episode, steps, ta}."""
        A, out = self.A, []
        for e in range(self.E):
            if self.ended[e]:   # lazy auto-reset at the start of the step: on_episode_start
                self.episode[e] += 1
                self.oracles[e], self.handlers[e], self.ended[e] = self._new(e), TimeAveragedStats(), False
            o = self.oracles[e]
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            self.handlers[e].on_step(oracle_game(self.prog, o))
            s = o.snapshot()
            early_end = self.early is not None and self.episode[e] == 0 and o.current_step >= self.early[e]
            self.ended[e] = bool(s["terminals"].all()) or bool(s["truncations"].all()) or early_end
            if self.ended[e]:
                out.append({"env": e, "episode": self.episode[e], "steps": o.current_step, "partial": False,
                            "ta": self.handlers[e].time_averaged_game_stats})
        return out


class HostTotals:
    """The engine's accumulation order restated (csrc/mgx_time_avg.h): per step the finished envs in ascending env index, in
    chunks of 256 whose sums (started from 0.0) are added to the totals in chunk order; partial episodes only counted."""

    def __init__(self, prog):
        self.names = list(prog.game_stat_names)
        self.clear()

    def clear(self):
        self.n = self.partial = 0
        self.sum = {k: 0.0 for k in self.names}
        self.cnt = {k: 0 for k in self.names}

    def add_step(self, finished: list):
        for c0 in range(0, len(finished), 256):
            s = {k: 0.0 for k in self.names}
            for f in finished[c0:c0 + 256]:
                if f["partial"]:
                    self.partial += 1
                    continue
                self.n += 1
                for k in self.names:
                    s[k] += f["ta"].get(k, 0.0)
                    self.cnt[k] += k in f["ta"]
            for k in self.names:
                self.sum[k] += s[k]

    def as_dict(self) -> dict:
        return {"episodes": self.n, "partial": self.partial, "sum": {k: v for k, v in self.sum.items() if self.cnt[k]},
                "count": {k: v for k, v in self.cnt.items() if v}}


def _same_totals(got: dict, want: dict, where: str) -> None:
    assert (got["episodes"], got["partial"], got["count"]) == (want["episodes"], want["partial"], want["count"]), (where, got, want)
    same_f64_dict(got["sum"], want["sum"], where)


def _same_records(recs: list, want: list, where: str) -> None:
    assert len(recs) == len(want), (where, len(recs), len(want))
    for r, x in zip(recs, want):
        w = f"{where} env {x['env']} episode {x['episode']}"
        assert (r["env"], r["episode"], r["steps"], r["partial"]) == (x["env"], x["episode"], x["steps"], x["partial"]), (w, r, x)
        assert r["ta_steps"] == x.get("ta_steps", x["steps"]), (w, r)
        same_f64_dict(r["time_averaged_game_stats"], x["ta"], w)


def _random_actions(rng, prog, E):
    n = len(prog.action_names)
    return rng.integers(0, n, E * prog.num_agents).astype(np.int32), rng.integers(0, n, E * prog.num_agents).astype(np.int32)


def _run(workload: str, E: int, steps: int, max_steps: int, drain_every: int = 37) -> int:
    prog, pool = _program(workload, max_steps)
    early = first_integers((11 + np.arange(E)).astype(np.uint32), max_steps)
    eng, seeds = _engine(prog, pool, E, early)
    mirror = Mirror(prog, pool, seeds, early)
    want, expected, n_eps = HostTotals(prog), [], 0
    rng = np.random.default_rng(5)
    for t in range(steps):
        a, v = _random_actions(rng, prog, E)
        eng.actions[:] = a
        eng.vibe_actions[:] = v
        eng.step()
        fin = mirror.step(a, v)
        want.add_step(fin)
        expected += fin
        n_eps += len(fin)
        if (t + 1) % drain_every == 0 or t == steps - 1:
            _same_totals(eng.drain_time_averages(), want.as_dict(), f"{workload} totals at step {t}")
            want.clear()
            recs, dropped = eng.drain_time_average_log()
            assert dropped == 0
            _same_records(recs, expected, workload)
            expected = []
    assert eng.poll_errors()[0] & ~2 == 0
    eng.close()
    return n_eps


@pytest.mark.parametrize("E,steps", [(3, 20), (70, 120)])
def test_time_averages_against_oracle_rung3(E, steps):
    """Rung-3 rules, 11-step episodes, 7-map pool, stride 3, desync: every finished episode's key set and f64 averages and
    every total.  70 envs: the flat (env, column) index crosses wavefront and workgroup boundaries and is no multiple of 64."""
    n = _run("rung3", E=E, steps=steps, max_steps=11)
    assert n >= E * (steps // 11)   # (no episode lasts longer than 11 steps)


def test_time_averages_extended_game():
    """Rung-4 preset: more game columns, territory / AoE stats that move mid-episode, values written by the values kernel."""
    n = _run("rung4", E=10, steps=30, max_steps=7, drain_every=11)
    assert n >= 30


def test_chunked_totals_when_every_env_finishes_at_once():
    """600 envs without desync all finish on the same step: three chunks (256 + 256 + 88) in the accumulation order."""
    prog, pool = _program("rung2", 6)
    E = 600
    eng, seeds = _engine(prog, pool, E, None, log=100, stride=1)
    mirror = Mirror(prog, pool, seeds, None, stride=1)
    rng = np.random.default_rng(1)
    want, fin = HostTotals(prog), []
    for t in range(6):
        a, _ = _random_actions(rng, prog, E)
        v = np.zeros_like(a)
        eng.actions[:] = a
        eng.vibe_actions[:] = v
        eng.step()
        fin = mirror.step(a, v)
    assert len(fin) == E
    want.add_step(fin)
    _same_totals(eng.drain_time_averages(), want.as_dict(), "three chunks")
    recs, dropped = eng.drain_time_average_log()
    assert dropped == 500
    _same_records(recs, fin[:100], "three chunks")
    assert eng.drain_time_averages()["episodes"] == 0
    eng.close()


def test_snapshot_protocol_two_windows():
    """fetch without a request is None; a request while one is pending changes nothing; the drain behind it is the pending
    snapshot (window 1) plus a fresh one (window 2); the totals are then as a cleared snapshot leaves them."""
    prog, pool = _program("rung2", 6)
    E = 5
    early = first_integers((11 + np.arange(E)).astype(np.uint32), 6)
    eng, seeds = _engine(prog, pool, E, early, log=0)
    mirror = Mirror(prog, pool, seeds, early)
    rng = np.random.default_rng(1)
    assert eng.fetch_time_averages(wait=False) is None

    def step(want):
        a, v = _random_actions(rng, prog, E)
        eng.actions[:] = a
        eng.vibe_actions[:] = v
        eng.step()
        want.add_step(mirror.step(a, v))

    w1, w2 = HostTotals(prog), HostTotals(prog)
    while w1.n == 0:
        step(w1)
    assert 0 < w1.n < E and max(mirror.episode) == 0, (w1.n, early)   # some, not all, envs have finished their first episode
    eng.request_time_averages()
    for _ in range(6):
        step(w2)
    assert w2.n >= E
    eng.request_time_averages()   # the first snapshot is still pending: nothing is taken, the totals keep accumulating
    a, b = w1.as_dict(), w2.as_dict()
    merged = {"episodes": a["episodes"] + b["episodes"], "partial": a["partial"] + b["partial"],
              "sum": {k: a["sum"].get(k, 0.0) + b["sum"].get(k, 0.0) for k in {**a["sum"], **b["sum"]}},
              "count": {k: a["count"].get(k, 0) + b["count"].get(k, 0) for k in {**a["count"], **b["count"]}}}
    _same_totals(eng.drain_time_averages(), merged, "two windows")
    _same_totals(eng.drain_time_averages(), HostTotals(prog).as_dict(), "cleared")
    assert eng.fetch_time_averages(wait=False) is None
    eng.close()


def test_feature_writes_no_engine_state():
    """Two engines, same seeds and actions, one with the feature on: digests, observations, rewards and the episode log are
    equal; after set_time_averages(False) the engine goes on as one that never had it."""
    prog, pool = _program("rung3", 11)
    E = 24
    early = first_integers((11 + np.arange(E)).astype(np.uint32), 11)
    on, _ = _engine(prog, pool, E, early)
    off, _ = _engine(prog, pool, E, early, ta=False)
    rng = np.random.default_rng(9)

    def both_step():
        a, v = _random_actions(rng, prog, E)
        for eng in (on, off):
            eng.actions[:] = a
            eng.vibe_actions[:] = v
            eng.step()
        assert np.array_equal(on.obs, off.obs) and np.array_equal(on.rewards, off.rewards)
        assert np.array_equal(on.terminals, off.terminals) and np.array_equal(on.truncations, off.truncations)

    def same_logs():
        assert np.array_equal(on.state_digests(), off.state_digests())
        (ra, da), (rb, db) = on.drain_episode_log(), off.drain_episode_log()
        assert da == db == 0 and len(ra) == len(rb) > 0
        for x, y in zip(ra, rb):
            assert (x["env"], x["episode"], x["steps"], x["flags"], x["game"], x["agent"]) == (y["env"], y["episode"], y["steps"], y["flags"], y["game"], y["agent"])
        ta, tb = on.drain_episode_stats(), off.drain_episode_stats()
        assert ta == tb

    for _ in range(40):
        both_step()
    same_logs()
    assert on.drain_time_averages()["episodes"] > 0
    on.set_time_averages(False)
    with pytest.raises(ValueError, match="time averages are off"):
        on.time_averages([0])
    for _ in range(12):
        both_step()
    same_logs()
    on.close(); off.close()


def test_refused_without_episode_statistics():
    prog, pool = _program("rung2", 6)
    eng = BatchedMettaGrid(prog, pool[:2], [1, 2], buffers="host")
    with pytest.raises(ValueError, match="episode statistics are off"):
        eng.set_time_averages(True)
    eng.set_episode_stats(True)
    eng.set_time_averages(True, log_capacity=3)
    assert eng._tal["LOG_CAPACITY"] == 3 and eng._tal["NG"] == len(prog.game_stat_names)
    eng.set_episode_stats(True)                       # re-configuring the statistics switches the averages off
    with pytest.raises(ValueError, match="time averages are off"):
        eng.request_time_averages() or eng.time_averages([0])
    eng.close()


def test_mid_episode_reads_and_host_driven_restarts():
    """time_averages(envs) after 1, 5 and n - 1 steps is the handler's property on the oracle; a reset_envs without a record
    leaves zeroed accumulators; episodes recorded through record_episodes carry the right averages."""
    prog, pool = _program("rung3", 11)
    E, A = 5, prog.num_agents
    seeds = (11 + np.arange(E)).astype(np.uint32)
    eng = BatchedMettaGrid(prog, pool[np.arange(E) % M], seeds, buffers="host")
    eng.set_episode_stats(True, log_capacity=8)
    eng.set_time_averages(True, log_capacity=8)
    oracles = [op.OracleSim(prog, pool[e % M], int(seeds[e])) for e in range(E)]
    handlers = [TimeAveragedStats() for _ in range(E)]
    for o in oracles:
        o.reinit_buffers()
    assert eng.time_averages(range(E)) == [{}] * E      # zero steps
    rng = np.random.default_rng(2)

    def step():
        a, v = _random_actions(rng, prog, E)
        eng.actions[:] = a
        eng.vibe_actions[:] = v
        eng.step()
        for e, o in enumerate(oracles):
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            handlers[e].on_step(oracle_game(prog, o))

    for t in range(1, 11):
        step()
        if t in (1, 5, 10):
            for e, got in zip((4, 0, 2), eng.time_averages([4, 0, 2])):   # (a list in no particular order)
                same_f64_dict(got, handlers[e].time_averaged_game_stats, f"env {e} after {t} steps")
        if t == 5:   # env 3 is restarted by the host without a record: its accumulators start over
            mask = np.zeros(E, np.uint8); mask[3] = 1
            eng.reset_envs(mask, pool[np.arange(E) % M], seeds)
            assert eng.time_averages([3]) == [{}]
            oracles[3], handlers[3] = op.OracleSim(prog, pool[3 % M], int(seeds[3])), TimeAveragedStats()
            oracles[3].reinit_buffers()
    step()   # step 11: envs 0, 1, 2, 4 truncate; env 3 has played 6 steps
    done = (eng.truncations.reshape(E, A).all(1) | eng.terminals.reshape(E, A).all(1)).astype(np.uint8)
    assert list(done) == [1, 1, 1, 0, 1]
    eng.record_episodes(done)
    recs, dropped = eng.drain_time_average_log()
    want = [{"env": e, "episode": 0, "steps": 11, "partial": False, "ta": handlers[e].time_averaged_game_stats} for e in (0, 1, 2, 4)]
    _same_records(recs, want, "record_episodes")
    tot = HostTotals(prog)
    tot.add_step(want)
    _same_totals(eng.drain_time_averages(), tot.as_dict(), "record_episodes totals")
    eng.reset_envs(done, pool[np.arange(E) % M], seeds)
    assert eng.time_averages([0, 1, 2, 4]) == [{}] * 4
    same_f64_dict(eng.time_averages([3])[0], handlers[3].time_averaged_game_stats, "env 3 untouched by the others' restart")
    eng.close()


def test_state_moves():
    """copy_envs: the fork continues the source's average; raw load_envs: partial, divided by its own count, left out of the
    totals; enabling mid-episode: partial."""
    prog, pool = _program("rung3", 9)
    E, A = 4, prog.num_agents
    eng, seeds = _engine(prog, pool, E, None)
    oracles = [op.OracleSim(prog, pool[e % M], int(seeds[e])) for e in range(E)]
    for o in oracles:
        o.reinit_buffers()
    handlers = [TimeAveragedStats() for _ in range(E)]
    late = TimeAveragedStats()   # attached to env 1's oracle behind step 4: what the loaded copy of env 1 accumulates
    rng = np.random.default_rng(4)
    for t in range(9):
        a, v = _random_actions(rng, prog, E)
        if t >= 4:   # env 2 plays env 0's actions, env 3 env 1's
            for x in (a, v):
                x[2 * A:3 * A] = x[0:A]
                x[3 * A:4 * A] = x[A:2 * A]
        eng.actions[:] = a
        eng.vibe_actions[:] = v
        eng.step()
        for e in (0, 1):
            oracles[e].step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            handlers[e].on_step(oracle_game(prog, oracles[e]))
        if t >= 4:
            late.on_step(oracle_game(prog, oracles[1]))
        if t == 3:
            eng.copy_envs([0], [2])
            eng.load_envs(eng.save_envs([1]), [3])
            assert eng.time_averages([3]) == [{}]
            same_f64_dict(eng.time_averages([2])[0], handlers[0].time_averaged_game_stats, "copied accumulators")
    recs, dropped = eng.drain_time_average_log()
    t0, t1 = handlers[0].time_averaged_game_stats, handlers[1].time_averaged_game_stats
    want = [{"env": 0, "episode": 0, "steps": 9, "partial": False, "ta": t0}, {"env": 1, "episode": 0, "steps": 9, "partial": False, "ta": t1},
            {"env": 2, "episode": 0, "steps": 9, "partial": False, "ta": t0},
            {"env": 3, "episode": 0, "steps": 9, "partial": True, "ta_steps": 5, "ta": late.time_averaged_game_stats}]
    _same_records(recs, want, "state moves")
    tot = HostTotals(prog)
    tot.add_step(want)
    assert tot.n == 3 and tot.partial == 1
    _same_totals(eng.drain_time_averages(), tot.as_dict(), "state moves totals")
    # enabling mid-episode: every env is 3 steps into its (second) episode when the accumulation starts
    eng.set_time_averages(False)
    for t in range(3):
        eng.actions[:], eng.vibe_actions[:] = _random_actions(rng, prog, E)
        eng.step()
    eng.set_time_averages(True, log_capacity=8)
    for t in range(6):
        eng.actions[:], eng.vibe_actions[:] = _random_actions(rng, prog, E)
        eng.step()
    recs, _ = eng.drain_time_average_log()
    assert [(r["env"], r["steps"], r["ta_steps"], r["partial"]) for r in recs] == [(e, 9, 6, True) for e in range(E)]
    tot = eng.drain_time_averages()
    assert tot["episodes"] == 0 and tot["partial"] == E and tot["sum"] == {}
    eng.close()


def test_wrapper_with_map_fn_joins_every_episode_of_an_env():
    """Host-driven restarts through the wrapper (map_fn): every env finishes two episodes before episode_infos() is called —
    the engine numbers both 0 there — and each entry carries its own episode's averages; infos has the batch's."""
    prog, _ = _program("rung2", 5)
    E, A = 3, prog.num_agents
    map_fn = lambda e, ep: prog.class_map(presets.rung2_map(100 * ep + e))  # noqa: E731
    env = MettaGridBatchedEnv(prog, E, map_fn=map_fn, seed=7, buffers="host", episode_log=16, time_averaged_stats=True)
    env.reset()

    def new(e, ep):
        o = op.OracleSim(prog, map_fn(e, ep), 7 + e)
        o.reinit_buffers()
        return o, TimeAveragedStats()

    mirror = [new(e, 0) for e in range(E)]
    episode, want, windows = [0] * E, [], []
    rng = np.random.default_rng(8)
    for t in range(12):
        if t in (5, 10):   # the wrapper finds every env truncated at the start of this step: record, then restart
            fin = [{"env": e, "steps": 5, "partial": False, "ta": mirror[e][1].time_averaged_game_stats} for e in range(E)]
            want.append(fin)
            for e in range(E):
                episode[e] += 1
                mirror[e] = new(e, episode[e])
        *_, infos = env.step(rng.integers(0, env.single_action_n, E * A).astype(np.int32))
        a, v = env.engine.actions.copy(), env.engine.vibe_actions.copy()
        for e, (o, h) in enumerate(mirror):
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            h.on_step(oracle_game(prog, o))
        if infos:
            windows.append((t, infos))
    assert [t for t, _ in windows] == [5, 10]
    for (_, infos), fin in zip(windows, want):
        tot = HostTotals(prog)
        tot.add_step(fin)
        assert infos["episodes"] == E and "time_averaged_partial" not in infos and infos["time_averaged_count"] == tot.as_dict()["count"]
        same_f64_dict(infos["time_averaged_game"], {k: s / E for k, s in tot.as_dict()["sum"].items()}, "map_fn window")
    entries = env.episode_infos()
    flat = [f for fin in want for f in fin]
    assert [(i["env"], i["attributes"]["steps"]) for i in entries] == [(f["env"], f["steps"]) for f in flat]
    for i, f in zip(entries, flat):
        same_f64_dict(i["time_averaged_game_stats"], f["ta"], f"map_fn env {f['env']}")
    # the two episodes of an env differ (other map): a join that kept one per env would have failed above
    assert any(np.float64(a["ta"][k]).tobytes() != np.float64(b["ta"][k]).tobytes() for a, b in zip(want[0], want[1]) for k in a["ta"] if k in b["ta"])
    env.close()


def _wrapper(prog, pool, E, **kw):
    return MettaGridBatchedEnv(prog, E, map_pool=pool, pool_stride=STRIDE, seed=11, validate_actions=False, time_averaged_stats=True, **kw)


def test_wrapper_save_and_load_state_resume_the_average():
    """save_state -> load_state into a fresh engine: the resumed episodes are not partial and bit-equal to the uninterrupted run."""
    prog, pool = _program("rung3", 9)
    E, A = 6, prog.num_agents
    one = _wrapper(prog, pool, E, buffers="host", episode_log=32)
    two = _wrapper(prog, pool, E, buffers="host", episode_log=32)
    one.reset(); two.reset()
    rng = np.random.default_rng(6)
    n = one.single_action_n
    for t in range(4):
        one.step(rng.integers(0, n, E * A).astype(np.int32))
    st = one.save_state()
    assert st.extra["time_avg"].dtype == np.uint32 and st.extra["time_avg"].shape[0] == E
    from mettagrid_amd.engine import EnvState
    two.load_state(EnvState.from_dict(st.to_dict()))
    for t in range(5):
        a = rng.integers(0, n, E * A).astype(np.int32)
        one.step(a); two.step(a)
    x, y = one.episode_infos(), two.episode_infos()
    assert len(x) == len(y) == E
    for p, q in zip(x, y):
        assert p["env"] == q["env"] and "time_averaged_partial" not in p and "time_averaged_partial" not in q
        assert p["attributes"]["steps"] == q["attributes"]["steps"] == 9
        assert p["time_averaged_game_stats"] and p["game"] == q["game"]
        same_f64_dict(q["time_averaged_game_stats"], p["time_averaged_game_stats"], f"resumed env {p['env']}")
    # without the accumulators the resumed episodes are flagged
    three = _wrapper(prog, pool, E, buffers="host", episode_log=32)
    three.reset()
    bare = EnvState(st.data, st.info, st.envs, {k: v for k, v in st.extra.items() if k != "time_avg"})
    three.load_state(bare)
    partial_windows = []
    for t in range(5):
        *_, infos = three.step(rng.integers(0, n, E * A).astype(np.int32))
        if infos:
            assert infos["episodes"] == E and "time_averaged_game" not in infos
            partial_windows.append(infos["time_averaged_partial"])
    assert all(i.get("time_averaged_partial") for i in three.episode_infos())
    assert partial_windows == [E]   # the aggregate says how many of its episodes are in neither time_averaged_game nor its divisor
    one.close(); two.close(); three.close()


def test_wrapper_infos_episode_infos_and_summary():
    """MettaGridBatchedEnv(time_averaged_stats=True): the aggregate's time_averaged_game is sum / episodes of the per-episode
    values in the documented order, every episode_infos() entry carries its dict, and summarize_episodes of those entries
    equals the reference's arithmetic over the oracles' handlers."""
    import torch
    prog, pool = _program("rung3", 8)
    E, A = 96, prog.num_agents
    env = _wrapper(prog, pool, E, desync=True, episode_log=4096, log_per_agent=True)
    env.reset()
    seeds = ((11 + np.arange(E)) & 0xFFFFFFFF).astype(np.uint32)
    mirror = Mirror(prog, pool, seeds, env.early_end_steps())
    g = torch.Generator(device="cuda").manual_seed(0)
    per_step, windows = [], []
    for t in range(60):
        a = torch.randint(0, env.transport_action_n, (E * A,), device="cuda", dtype=torch.int32, generator=g)
        *_, rew, _, _, infos = env.step(a)
        float(rew.sum())   # a consumer reads the step's results
        per_step.append(mirror.step(env.engine.actions.cpu().numpy(), env.engine.vibe_actions.cpu().numpy()))
        if infos:
            assert set(infos) >= {"episodes", "game", "time_averaged_game", "time_averaged_count"}
            windows.append(infos)
    env.engine.sync()
    assert len(windows) >= 10
    # a window holds whole steps, oldest first: its totals are those steps' chunk sums added in step order
    it = iter(per_step)
    for w in windows:
        tot, n = HostTotals(prog), 0
        while n < w["episodes"]:
            fin = next(it)
            tot.add_step(fin)
            n += len(fin)
        assert n == w["episodes"]
        d = tot.as_dict()
        assert w["time_averaged_count"] == d["count"]
        same_f64_dict(w["time_averaged_game"], {k: v / n for k, v in d["sum"].items()}, "window")
    mirrored = [f for fin in per_step for f in fin]
    per_episode = env.episode_infos()
    assert len(per_episode) == len(mirrored) and env.episodes_dropped == 0
    for info, f in zip(per_episode, mirrored):
        assert (info["env"], info["episode"], info["attributes"]["steps"]) == (f["env"], f["episode"], f["steps"])
        same_f64_dict(info["time_averaged_game_stats"], f["ta"], f"env {f['env']} episode {f['episode']}")
    s = summarize_episodes(per_episode, [i % 2 for i in range(A)], 2)
    summed = {}
    for f in mirrored:   # summary.py:58-59, 72-74
        for k, v in f["ta"].items():
            summed[k] = summed.get(k, 0.0) + float(v)
    same_f64_dict(s["avg_time_averaged_game_stats"], {k: v / len(mirrored) for k, v in summed.items()}, "summary")
    assert s["episodes"] == len(mirrored) and sum(p["agent_count"] for p in s["policy_summaries"]) == A
    # with the argument off, infos and episode_infos() carry nothing of it
    plain = MettaGridBatchedEnv(prog, 8, map_pool=pool, pool_stride=STRIDE, seed=11, validate_actions=False, episode_log=64, buffers="host")
    plain.reset()
    for t in range(10):
        *_, infos = plain.step(np.zeros(8 * A, np.int32))
        assert "time_averaged_game" not in infos
    assert all("time_averaged_game_stats" not in i for i in plain.episode_infos())
    plain.close(); env.close()
