"""GPU: per-policy episode statistics, reduced on the device (include/mgx.h "Per-policy episode statistics"; the reference's
build_multi_episode_rollout_summaries, python/src/mettagrid/simulator/multi_episode/summary.py:38-130).  Every env is mirrored
by an oracle env whose per-agent stat dicts and episode rewards at each episode end are the source of truth; the expected
records are computed from them with plain Python floats in agent order and the expected totals in the engine's restated
chunk order (tests/test_policy_summary_fixture.py: policy_record, PolicyHostTotals), and compared bit for bit."""
import numpy as np
import pytest

import oracle_py as op
from helpers import reference_infos
from mettagrid_amd.early_reset import first_integers
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv
from mettagrid_amd.summary import summarize_episodes, summarize_policy_totals
from test_gpu_time_avg import M, STRIDE, _program, _random_actions
from test_policy_summary_fixture import PolicyHostTotals, policy_record

pytestmark = pytest.mark.gpu

MAXP = BatchedMettaGrid.MAX_POLICIES


def _engine(prog, pool, E, early, rows, P, log=None, stride=STRIDE, auto=True, per_agent=False, ta=False):
    seeds = (11 + np.arange(E)).astype(np.uint32)
    eng = BatchedMettaGrid(prog, pool[np.arange(E) % M], seeds, buffers="host")
    if auto:
        eng.set_map_pool(pool)
        eng.set_auto_reset(True, stride, early)
    log = 16 * E if log is None else log
    eng.set_episode_stats(True, log_capacity=log, log_per_agent=per_agent)
    if ta:
        eng.set_time_averages(True, log_capacity=log)
    if rows is not None:
        eng.set_policy_stats(True, P, rows, log_capacity=log)
    return eng, seeds


def _new_oracle(prog, cells, seed):
    o = op.OracleSim(prog, cells, int(seed))
    o.reinit_buffers()
    return o


def _finished(prog, o, env, episode, row, P, early_end=False) -> dict:
    """The expected record of an oracle env whose episode ends now under the assignment row ``row``."""
    s = o.snapshot()
    info = reference_infos(prog, o)
    per_agent = [info["per_agent"][str(i)] for i in range(prog.num_agents)]
    rec = policy_record(per_agent, info["episode_rewards"], row, P)
    all_term, all_trunc = bool(s["terminals"].all()), bool(s["truncations"].all()) or early_end
    rec.update(env=env, episode=episode, steps=o.current_step, flags=(1 if all_term else 0) | (2 if all_trunc else 0) | (4 if early_end else 0),
               per_agent=per_agent, rewards=info["episode_rewards"], row=[int(x) for x in row])
    return rec


class Mirror:
    """One oracle env per engine env, restarted when the engine's auto-reset restarts it; ``rows``: the assignment table
    (changed by the test when it changes the engine's)."""

    def __init__(self, prog, pool, seeds, early, rows, P, stride=STRIDE):
        self.prog, self.pool, self.seeds, self.early, self.stride, self.P = prog, pool, seeds, early, stride, P
        self.E, self.A = len(seeds), prog.num_agents
        self.rows = np.array(np.broadcast_to(np.asarray(rows), (self.E, self.A)), dtype=np.uint8)
        self.episode, self.ended = [0] * self.E, [False] * self.E
        self.oracles = [self._new(e) for e in range(self.E)]

    def _new(self, e):
        return _new_oracle(self.prog, self.pool[(e + self.episode[e] * self.stride) % len(self.pool)], self.seeds[e])

    def step(self, a, v) -> list:
        """-> the expected records of this step's finished episodes, in ascending env index."""
        A, out = self.A, []
        for e in range(self.E):
            if self.ended[e]:   # lazy auto-reset at the start of the step
                self.episode[e] += 1
                self.oracles[e], self.ended[e] = self._new(e), False
            o = self.oracles[e]
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
            s = o.snapshot()
            early_end = self.early is not None and self.episode[e] == 0 and o.current_step >= self.early[e]
            self.ended[e] = bool(s["terminals"].all()) or bool(s["truncations"].all()) or early_end
            if self.ended[e]:
                out.append(_finished(self.prog, o, e, self.episode[e], self.rows[e], self.P, early_end))
        return out


def _bits(x) -> bytes:
    return np.float64(x).tobytes()


def _same_f64_dict(got: dict, want: dict, where) -> None:
    assert got.keys() == want.keys(), (where, sorted(set(got) ^ set(want)))
    for k in got:
        assert _bits(got[k]) == _bits(want[k]), (where, k, got[k], want[k])


def _same_records(recs: list, want: list, where: str) -> None:
    assert len(recs) == len(want), (where, len(recs), len(want))
    for r, x in zip(recs, want):
        w = f"{where} env {x['env']} episode {x['episode']}"
        assert (r["env"], r["episode"], r["steps"], r["flags"]) == (x["env"], x["episode"], x["steps"], x["flags"]), (w, r, x)
        assert list(r["agents"]) == x["agents"], w
        assert [_bits(v) for v in r["reward_sum"]] == [_bits(v) for v in x["reward_sum"]], (w, r["reward_sum"], x["reward_sum"])
        assert [None if v is None else _bits(v) for v in r["avg_rewards"]] == [None if v is None else _bits(v) for v in x["avg_rewards"]], w
        for p, (g, h) in enumerate(zip(r["policies"], x["policies"])):
            _same_f64_dict(g, h, (w, "policy", p))   # key sets = the exists bits, values = the sums


def _same_totals(got: dict, want: dict, where: str) -> None:
    assert got["episodes"] == want["episodes"] and len(got["policies"]) == len(want["policies"]), (where, got["episodes"], want["episodes"])
    for p, (g, w) in enumerate(zip(got["policies"], want["policies"])):
        assert (g["episodes"], g["agent_episodes"], g["agent_count"]) == (w["episodes"], w["agent_episodes"], w["agent_count"]), (where, p, g, w)
        for k in ("avg_reward_sum", "avg_reward_min", "avg_reward_max"):
            assert _bits(g[k]) == _bits(w[k]), (where, p, k, g[k], w[k])
        _same_f64_dict(g["agent_sum"], w["agent_sum"], (where, p))


def _play(eng, a, v):
    eng.actions[:] = a
    eng.vibe_actions[:] = v
    eng.step()


def _run(workload, E, steps, max_steps, rows, P, drain_every=37, per_agent=False):
    """-> (every expected record, the windows' totals dicts, the episode log's records with per_agent)."""
    prog, pool = _program(workload, max_steps)
    early = first_integers((11 + np.arange(E)).astype(np.uint32), max_steps)
    eng, seeds = _engine(prog, pool, E, early, rows, P, per_agent=per_agent)
    mirror = Mirror(prog, pool, seeds, early, rows, P)
    want, expected, every, windows, ep_log = PolicyHostTotals(prog.agent_stat_names, P), [], [], [], []
    rng = np.random.default_rng(5)
    for t in range(steps):
        a, v = _random_actions(rng, prog, E)
        _play(eng, a, v)
        fin = mirror.step(a, v)
        want.add_step(fin)
        expected += fin
        if (t + 1) % drain_every == 0 or t == steps - 1:
            got = eng.drain_policy_stats()
            _same_totals(got, want.as_dict(), f"{workload} totals at step {t}")
            windows.append(got)
            want.clear()
            recs, dropped = eng.drain_policy_log()
            assert dropped == 0
            _same_records(recs, expected, workload)
            every += expected
            expected = []
            if per_agent:
                ep_log += eng.drain_episode_log()[0]
    assert eng.poll_errors()[0] & ~2 == 0
    eng.close()
    return every, windows, ep_log


@pytest.mark.parametrize("E,steps", [(3, 20), (70, 120)])
def test_two_policies_against_oracle_rung3(E, steps):
    """Rung-3 rules (16 agents, 86 stat columns: two column blocks), 11-step episodes, 7-map pool, desync, policies alternating
    over the agent rows: every log record and every total.  3 envs: a partial wavefront of the done list; 70: more than 64."""
    A = 16
    every, _, _ = _run("rung3", E, steps, 11, [i % 2 for i in range(A)], 2)
    assert len(every) >= E * (steps // 11)
    assert all(r["agents"] == [8, 8] for r in every) and any(r["policies"][0] != r["policies"][1] for r in every)


def test_extended_game_three_policies_and_the_summary():
    """Rung-4 preset (64 agents, 92 stat columns), a different row per env: env 1 gives policy 2 no agent, env 2's row is a
    permutation of env 0's.  Besides records and totals: summarize_episodes over the per-agent log of the same run against
    summarize_policy_totals over the windows' totals — equal bit for bit in every (policy, key) whose addends are all integers
    (any order of an integer sum below 2^53 is exact); for any other, the two undivided sums (the reference's order: episodes
    outermost; the device's: per episode, then per chunk, then per window) differ by at most 2 (m - 1) 2^-53 sum|addends| over
    the m addends, the bound for two orderings of one f64 sum."""
    A, P = 64, 3
    base = np.array([i % 3 for i in range(A)], np.uint8)
    rows = np.stack([base, np.array([i % 2 for i in range(A)], np.uint8), base[::-1].copy(), np.array([(i // 8) % 3 for i in range(A)], np.uint8)])
    assert sorted(rows[2]) == sorted(rows[0]) and (rows[2] != rows[0]).any() and 2 not in rows[1]
    every, windows, ep_log = _run("rung4", 4, 30, 7, rows, P, drain_every=11, per_agent=True)
    assert len(every) >= 12 and any(r["env"] == 1 and r["avg_rewards"][2] is None for r in every)
    assert len(ep_log) == len(every) and [(r["env"], r["steps"]) for r in ep_log] == [(x["env"], x["steps"]) for x in every]
    asg = [[int(p) for p in rows[r["env"]]] for r in ep_log]
    ref = summarize_episodes(ep_log, asg, P)
    dev = summarize_policy_totals(windows, asg[0])
    assert dev["episodes"] == ref["episodes"] == len(every)
    n_exact = n_bounded = 0
    for p in range(P):
        rp, dp = ref["policy_summaries"][p], dev["policy_summaries"][p]
        assert rp["agent_count"] == dp["agent_count"] == asg[0].count(p) and list(rp["avg_agent_metrics"]) == list(dp["avg_agent_metrics"])
        assert dp["agent_episodes"] == sum(a.count(p) for a in asg)
        for key in rp["avg_agent_metrics"]:
            addends = [float(r["per_agent"][i][key]) for r, a in zip(ep_log, asg) for i in range(A) if a[i] == p and key in r["per_agent"][i]]
            if all(x == int(x) for x in addends) and sum(abs(x) for x in addends) < 2.0 ** 53:
                assert _bits(rp["avg_agent_metrics"][key]) == _bits(dp["avg_agent_metrics"][key]), (p, key)
                n_exact += 1
            else:
                s_ref = 0.0
                for x in addends:
                    s_ref += x
                s_dev = 0.0
                for w in windows:
                    s_dev += w["policies"][p]["agent_sum"].get(key, 0.0)
                assert abs(s_ref - s_dev) <= 2 * (len(addends) - 1) * 2.0 ** -53 * sum(abs(x) for x in addends), (p, key, s_ref, s_dev)
                n_bounded += 1
    assert n_exact > 0
    # the per-episode reward rows of the reference's summary are the records' rows
    for i, x in enumerate(every):
        assert [None if v is None else _bits(v) for v in ref["per_episode_per_policy_avg_rewards"][i]] == [None if v is None else _bits(v) for v in x["avg_rewards"]]


def test_chunked_totals_when_every_env_finishes_at_once():
    """600 envs without desync all finish on the same step: three chunks (256 + 256 + 88) in the accumulation order; the log
    holds the first 100 records and counts the rest."""
    prog, pool = _program("rung2", 6)
    E, A, P = 600, prog.num_agents, 2
    rows = np.array([[(i + e) % 2 if e % 3 else (i // 4) % 2 for i in range(A)] for e in range(E)], np.uint8)
    eng, seeds = _engine(prog, pool, E, None, rows, P, log=100, stride=1)
    mirror = Mirror(prog, pool, seeds, None, rows, P, stride=1)
    rng = np.random.default_rng(1)
    fin = []
    for t in range(6):
        a, _ = _random_actions(rng, prog, E)
        v = np.zeros_like(a)
        _play(eng, a, v)
        fin = mirror.step(a, v)
    assert len(fin) == E
    want = PolicyHostTotals(prog.agent_stat_names, P)
    want.add_step(fin)
    _same_totals(eng.drain_policy_stats(), want.as_dict(), "three chunks")
    recs, dropped = eng.drain_policy_log()
    assert dropped == 500
    _same_records(recs, fin[:100], "three chunks")
    assert eng.drain_policy_stats()["episodes"] == 0
    eng.close()


def _merged(w1: dict, w2: dict) -> dict:
    """Two windows' totals as one: sums and counts add, minima take min, maxima take max."""
    def policy(x, y):
        out = {k: x[k] + y[k] for k in ("episodes", "agent_episodes", "avg_reward_sum")}
        out["avg_reward_min"], out["avg_reward_max"] = min(x["avg_reward_min"], y["avg_reward_min"]), max(x["avg_reward_max"], y["avg_reward_max"])
        for k in ("agent_sum", "agent_count"):
            out[k] = {n: x[k].get(n, 0) + y[k].get(n, 0) for n in {**x[k], **y[k]}}
        return out
    return {"episodes": w1["episodes"] + w2["episodes"], "policies": [policy(x, y) for x, y in zip(w1["policies"], w2["policies"])]}


def test_snapshot_protocol_two_windows():
    """fetch without a request is None; a request while one is pending changes nothing; the drain behind it is the pending
    snapshot (window 1) merged with a fresh one (window 2); the totals are then as a cleared snapshot leaves them."""
    prog, pool = _program("rung2", 6)
    E, A, P = 5, prog.num_agents, 2
    rows = np.array([[(i + e) % 2 if e % 3 else (i // 4) % 2 for i in range(A)] for e in range(E)], np.uint8)
    early = first_integers((11 + np.arange(E)).astype(np.uint32), 6)
    eng, seeds = _engine(prog, pool, E, early, rows, P, log=0)
    mirror = Mirror(prog, pool, seeds, early, rows, P)
    rng = np.random.default_rng(1)
    assert eng.fetch_policy_stats(wait=False) is None

    def step(want):
        a, v = _random_actions(rng, prog, E)
        _play(eng, a, v)
        want.add_step(mirror.step(a, v))

    w1, w2 = PolicyHostTotals(prog.agent_stat_names, P), PolicyHostTotals(prog.agent_stat_names, P)
    while w1.n == 0:
        step(w1)
    assert 0 < w1.n < E and max(mirror.episode) == 0, (w1.n, early)   # some, not all, envs have finished their first episode
    eng.request_policy_stats()
    for _ in range(6):
        step(w2)
    assert w2.n >= E
    eng.request_policy_stats()   # the first snapshot is still pending: nothing is taken, the totals keep accumulating
    _same_totals(eng.drain_policy_stats(), _merged(w1.as_dict(), w2.as_dict()), "two windows")
    empty = eng.drain_policy_stats()
    _same_totals(empty, PolicyHostTotals(prog.agent_stat_names, P).as_dict(), "cleared")
    assert empty["episodes"] == 0 and all(p["avg_reward_min"] == np.inf and p["avg_reward_max"] == -np.inf for p in empty["policies"])
    assert eng.fetch_policy_stats(wait=False) is None
    eng.close()


def test_most_policies_and_refusals():
    """MGX_MAX_POLICIES policies: env 0 and 2 give every policy one agent, env 1 spreads its agents over the first 8 (the
    rest have none).  One policy more, and an assignment >= P, are refused with MGX_ERR_BAD_ARG — by set_policy_stats and by
    set_policy_assignments — and the table set before stays in force."""
    prog, pool = _program("rung3", 11)
    E, A, P = 3, prog.num_agents, MAXP
    assert A == MAXP
    rows = np.array([list(range(A)), [i % 8 for i in range(A)], list(range(A))[::-1]], np.uint8)
    eng, seeds = _engine(prog, pool, E, None, rows, P)
    mirror = Mirror(prog, pool, seeds, None, rows, P)
    rng = np.random.default_rng(3)
    want, fin = PolicyHostTotals(prog.agent_stat_names, P), []
    for t in range(11):
        if t == 4:
            with pytest.raises(ValueError, match="policies"):
                eng.set_policy_stats(True, MAXP + 1, rows)
            with pytest.raises(ValueError, match="policies"):
                eng.set_policy_stats(True, 0, rows)
            bad = rows.copy()
            bad[2, 5] = MAXP
            with pytest.raises(ValueError, match=f"row 2, agent 5: policy {MAXP} of {MAXP}"):
                eng.set_policy_stats(True, MAXP, bad)
            with pytest.raises(ValueError, match="row 0, agent 8: policy 8 of 8"):
                eng.set_policy_stats(True, 8, rows)
            with pytest.raises(ValueError, match=f"policy {MAXP} of {MAXP}"):
                eng.set_policy_assignments([2], bad[2])
            with pytest.raises(ValueError):
                eng.set_policy_assignments([1, 1], rows[:2])
            assert eng._psl["P"] == MAXP
        a, v = _random_actions(rng, prog, E)
        _play(eng, a, v)
        fin = mirror.step(a, v)
    assert len(fin) == E and fin[1]["avg_rewards"][8:] == [None] * 8 and fin[0]["agents"] == [1] * MAXP
    want.add_step(fin)
    recs, dropped = eng.drain_policy_log()
    _same_records(recs, fin, "16 policies")
    _same_totals(eng.drain_policy_stats(), want.as_dict(), "16 policies")
    eng.close()


def test_set_policy_assignments_between_episodes():
    """Rows replaced behind an episode's end: that episode keeps the old attribution, the next one has the new; rows of envs
    not listed are unchanged."""
    prog, pool = _program("rung3", 5)
    E, A, P = 4, prog.num_agents, 2
    old = np.array([i % 2 for i in range(A)], np.uint8)
    eng, seeds = _engine(prog, pool, E, None, old, P)
    mirror = Mirror(prog, pool, seeds, None, old, P)
    new = np.array([[1] * 4 + [0] * 12, [(i // 2) % 2 for i in range(A)]], np.uint8)
    rng = np.random.default_rng(7)
    expected = []
    for t in range(10):
        a, v = _random_actions(rng, prog, E)
        _play(eng, a, v)
        expected += mirror.step(a, v)
        if t == 4:   # (every env has just finished its first episode)
            assert len(expected) == E
            eng.set_policy_assignments([3, 1], new)
            mirror.rows[3], mirror.rows[1] = new[0], new[1]
    assert len(expected) == 2 * E
    assert [x["row"] for x in expected[E:]] == [list(old), list(new[1]), list(old), list(new[0])] and expected[E + 3]["agents"] == [12, 4]
    recs, dropped = eng.drain_policy_log()
    assert dropped == 0
    _same_records(recs, expected, "rematched")
    eng.close()


def test_table_belongs_to_the_slot():
    """copy_envs and save_envs / load_envs into another slot move the episode, not the row: the destination's episode ends
    under the destination's row; the saved record's size does not change with the feature."""
    prog, pool = _program("rung3", 9)
    E, A, P = 4, prog.num_agents, 2
    rows = np.array([[i % 2 for i in range(A)], [(i // 2) % 2 for i in range(A)], [1 - i % 2 for i in range(A)], [int(i < 5) for i in range(A)]], np.uint8)
    eng, seeds = _engine(prog, pool, E, None, None, P)
    before = eng.env_state_info()
    eng.set_policy_stats(True, P, rows, log_capacity=16)
    assert eng.env_state_info() == before
    oracles = [_new_oracle(prog, pool[e % M], seeds[e]) for e in range(2)]
    rng = np.random.default_rng(4)
    for t in range(9):
        a, v = _random_actions(rng, prog, E)
        if t >= 4:   # env 2 plays env 0's actions, env 3 env 1's
            for x in (a, v):
                x[2 * A:3 * A] = x[0:A]
                x[3 * A:4 * A] = x[A:2 * A]
        _play(eng, a, v)
        for e in (0, 1):
            oracles[e].step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
        if t == 3:
            eng.copy_envs([0], [2])
            eng.load_envs(eng.save_envs([1]), [3])
    want = [_finished(prog, oracles[src], env, 0, rows[env], P) for env, src in ((0, 0), (1, 1), (2, 0), (3, 1))]
    recs, dropped = eng.drain_policy_log()
    _same_records(recs, want, "slot-owned")
    assert want[0]["policies"] != want[2]["policies"]   # (the same episode under two rows)
    tot = PolicyHostTotals(prog.agent_stat_names, P)
    tot.add_step(want)
    _same_totals(eng.drain_policy_stats(), tot.as_dict(), "slot-owned totals")
    eng.close()


def test_off_means_off():
    """Two engines, same seeds and actions; one has the feature on for 25 steps and off again: layout words, episode totals
    and log, time-average totals and digests are those of the engine that never had it."""
    prog, pool = _program("rung3", 11)
    E, A = 24, prog.num_agents
    early = first_integers((11 + np.arange(E)).astype(np.uint32), 11)
    on, _ = _engine(prog, pool, E, early, [i % 2 for i in range(A)], 2, ta=True)
    off, _ = _engine(prog, pool, E, early, None, 2, ta=True)
    rng = np.random.default_rng(9)
    for t in range(40):
        a, v = _random_actions(rng, prog, E)
        for eng in (on, off):
            _play(eng, a, v)
        assert np.array_equal(on.obs, off.obs) and np.array_equal(on.rewards, off.rewards)
        if t == 24:
            assert on.drain_policy_stats()["episodes"] > 0
            on.set_policy_stats(False)
            with pytest.raises(ValueError, match="policy statistics are off"):
                on.drain_policy_stats()
    assert on._epl == off._epl and on._tal == off._tal
    assert np.array_equal(on.state_digests(), off.state_digests())
    (ra, da), (rb, db) = on.drain_episode_log(), off.drain_episode_log()
    assert da == db == 0 and len(ra) == len(rb) > 0
    for x, y in zip(ra, rb):
        assert (x["env"], x["episode"], x["steps"], x["flags"], x["game"], x["agent"]) == (y["env"], y["episode"], y["steps"], y["flags"], y["game"], y["agent"])
        assert np.array_equal(x["episode_rewards"], y["episode_rewards"])
    assert on.drain_episode_stats() == off.drain_episode_stats()
    assert on.drain_time_averages() == off.drain_time_averages()
    # setting the episode statistics again switches the feature off
    on.set_policy_stats(True, 2, [i % 2 for i in range(A)])
    on.set_episode_stats(True)
    with pytest.raises(ValueError, match="policy statistics are off"):
        on.request_policy_stats()
    assert on.L.mgx_request_policy_stats(on.h) == -1   # MGX_ERR_BAD_ARG
    # ... and it needs them
    on.set_episode_stats(False)
    with pytest.raises(ValueError, match="episode statistics are off"):
        on.set_policy_stats(True, 2, [i % 2 for i in range(A)])
    on.close(); off.close()


def test_host_driven_restarts_record_the_masked_envs():
    prog, pool = _program("rung3", 11)
    E, A, P = 5, prog.num_agents, 3
    rows = np.array([[(i + e) % 3 for i in range(A)] for e in range(E)], np.uint8)
    eng, seeds = _engine(prog, pool, E, None, rows, P, auto=False)
    oracles = [_new_oracle(prog, pool[e % M], seeds[e]) for e in range(E)]
    rng = np.random.default_rng(2)
    for t in range(6):
        a, v = _random_actions(rng, prog, E)
        _play(eng, a, v)
        for e, o in enumerate(oracles):
            o.step(a[e * A:(e + 1) * A], v[e * A:(e + 1) * A])
    eng.record_episodes(np.array([1, 0, 1, 1, 0], np.uint8))
    want = [_finished(prog, oracles[e], e, 0, rows[e], P) for e in (0, 2, 3)]
    recs, dropped = eng.drain_policy_log()
    _same_records(recs, want, "record_episodes")
    tot = PolicyHostTotals(prog.agent_stat_names, P)
    tot.add_step(want)
    _same_totals(eng.drain_policy_stats(), tot.as_dict(), "record_episodes totals")
    eng.close()


def test_wrapper_infos_episode_infos_and_rows():
    """MettaGridBatchedEnv(policy_assignments=...): infos["policy"] has the documented keys, every episode_infos() entry
    carries its row and the reference's per-policy reward row (summarize_episodes over the same entries), over two drains;
    policy_rows partition the agent rows.  Without the argument nothing of it appears."""
    import torch
    prog, pool = _program("rung3", 8)
    E, A = 12, prog.num_agents
    asg = [i % 2 for i in range(A)]
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, pool_stride=STRIDE, seed=11, validate_actions=False, desync=True, episode_log=512,
                              log_per_agent=True, policy_assignments=asg)
    env.reset()
    assert env.num_policies == 2
    r0, r1 = env.policy_rows(0), env.policy_rows(1)
    assert torch.equal(torch.sort(torch.cat([r0, r1])).values, torch.arange(E * A, device=r0.device)) and len(r0) == len(r1)
    assert env.policy_ids.dtype == torch.int64 and bool((env.policy_ids[r1] == 1).all())
    g = torch.Generator(device="cuda").manual_seed(0)
    n_policy_eps, n_entries = 0, 0
    for window in range(2):
        for t in range(20):
            a = torch.randint(0, env.transport_action_n, (E * A,), device="cuda", dtype=torch.int32, generator=g)
            *_, rew, _, _, infos = env.step(a)
            float(rew.sum())
            if infos:
                assert len(infos["policy"]) == 2
                for p in infos["policy"]:
                    assert set(p) == {"episodes", "agent_episodes", "avg_reward", "agent_sum", "agent_count"}
                    assert p["episodes"] == infos["episodes"] and p["agent_episodes"] == 8 * p["episodes"]
                    assert set(p["avg_reward"]) == {"mean", "min", "max"} and p["avg_reward"]["min"] <= p["avg_reward"]["mean"] <= p["avg_reward"]["max"]
                    assert p["agent_sum"].keys() == p["agent_count"].keys() and p["agent_sum"]
                n_policy_eps += infos["policy"][0]["episodes"]
        if window == 0:   # env 5 is rematched: its later episodes carry the new row
            env.set_policy_assignments([5], [1 - x for x in asg])
            assert bool((env.policy_ids[5 * A:6 * A] == torch.tensor([1 - x for x in asg], device=r0.device)).all())
        entries = env.episode_infos()
        n_entries += len(entries)
        assert len(entries) >= E and env.episodes_dropped == 0
        rows = [i["assignments"] for i in entries]
        if window == 0:
            assert all(r == asg for r in rows)
        else:
            assert all(r == ([1 - x for x in asg] if i["env"] == 5 else asg) for r, i in zip(rows, entries)) and any(i["env"] == 5 for i in entries)
        s = summarize_episodes(entries, rows, 2)
        for k, i in enumerate(entries):
            assert [_bits(x) for x in i["policy_avg_rewards"]] == [_bits(x) for x in s["per_episode_per_policy_avg_rewards"][k]]
    env.engine.sync()
    assert n_policy_eps + env.engine.drain_policy_stats()["policies"][0]["episodes"] == n_entries + len(env.episode_infos())
    env.close()
    plain = MettaGridBatchedEnv(prog, 4, map_pool=pool, pool_stride=STRIDE, seed=11, validate_actions=False, episode_log=64, buffers="host")
    plain.reset()
    for t in range(10):
        *_, infos = plain.step(np.zeros(4 * A, np.int32))
        assert "policy" not in infos
    assert all("assignments" not in i and "policy_avg_rewards" not in i for i in plain.episode_infos())
    with pytest.raises(ValueError, match="no policy_assignments"):
        plain.policy_rows(0)
    plain.close()
