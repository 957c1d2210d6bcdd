"""Host only: summary.py against the reference's own build_multi_episode_rollout_summaries
(python/src/mettagrid/simulator/multi_episode/summary.py:38-130), whose output over episodes built from the committed
infos_* / time_avg_* fixtures is tests/golden/policy_summary.json (tests/golden/make_policy_summary_fixture.py).

``policy_record`` and ``PolicyHostTotals`` restate what the device computes (csrc/mgx_policy_stats.h) with plain Python floats;
tests/test_gpu_policy_stats.py compares the engine with them."""
import json
import math
import os

import pytest

from mettagrid_amd.summary import summarize_episodes, summarize_policy_totals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "policy_summary.json")))
CHUNK = 256   # MGX_EP_CHUNK


def policy_record(per_agent: list, rewards, assignments, P: int) -> dict:
    """One episode's record: per policy {key: f64 sum over its agents in agent order, from +0.0} (a key exists when some
    agent of the policy holds it), the f64 sum of its agents' episode rewards in agent order and their number."""
    sums, rew, cnt = [dict() for _ in range(P)], [0.0] * P, [0] * P
    for a, (stats, r) in enumerate(zip(per_agent, rewards)):
        p = int(assignments[a])
        for k, v in stats.items():
            sums[p][k] = sums[p].get(k, 0.0) + float(v)
        rew[p] += float(r)
        cnt[p] += 1
    return {"policies": sums, "reward_sum": rew, "agents": cnt,
            "avg_rewards": [rew[p] / cnt[p] if cnt[p] else None for p in range(P)]}


class PolicyHostTotals:
    """The engine's accumulation order restated (csrc/mgx_policy_stats.h): per step the finished envs' records in list order,
    in chunks of 256 whose sums (started from 0.0) are added to the totals in chunk order; an episode in which a policy has
    no agent is in none of that policy's header words."""

    def __init__(self, names, P: int):
        self.names, self.P = list(names), P
        self.clear()

    def clear(self):
        self.n = 0
        self.pol = [{"episodes": 0, "agent_episodes": 0, "avg_reward_sum": 0.0, "avg_reward_min": math.inf, "avg_reward_max": -math.inf,
                     "sum": {k: 0.0 for k in self.names}, "cnt": {k: 0 for k in self.names}} for _ in range(self.P)]

    def add_step(self, records: list):
        for c0 in range(0, len(records), CHUNK):
            chunk = records[c0:c0 + CHUNK]
            self.n += len(chunk)
            for p, T in enumerate(self.pol):
                s, rs = {k: 0.0 for k in self.names}, 0.0
                for r in chunk:
                    held = r["policies"][p]
                    for k in self.names:
                        s[k] += held.get(k, 0.0)
                        T["cnt"][k] += k in held
                    if r["agents"][p]:
                        avg = r["reward_sum"][p] / r["agents"][p]
                        rs += avg
                        T["episodes"] += 1
                        T["agent_episodes"] += r["agents"][p]
                        T["avg_reward_min"], T["avg_reward_max"] = min(T["avg_reward_min"], avg), max(T["avg_reward_max"], avg)
                for k in self.names:
                    T["sum"][k] += s[k]
                T["avg_reward_sum"] += rs

    def as_dict(self) -> dict:
        """The shape of BatchedMettaGrid.policy_totals_dict."""
        return {"episodes": self.n,
                "policies": [{"episodes": T["episodes"], "agent_episodes": T["agent_episodes"], "avg_reward_sum": T["avg_reward_sum"],
                              "avg_reward_min": T["avg_reward_min"], "avg_reward_max": T["avg_reward_max"],
                              "agent_sum": {k: v for k, v in T["sum"].items() if T["cnt"][k]},
                              "agent_count": {k: v for k, v in T["cnt"].items() if v}} for T in self.pol]}


def episode_inputs(case: dict, k: int) -> dict:
    """Episode k of a case (make_policy_summary_fixture.py: the fixture's episode with its agents rotated by rotate[k] rows)."""
    infos = json.load(open(os.path.join(GOLDEN, f"infos_{case['scenario']}.json")))
    ta = json.load(open(os.path.join(GOLDEN, f"time_avg_{case['scenario']}.json")))
    A, r = len(infos["per_agent"]), case["rotate"][k]
    return {"game": infos["game"], "per_agent": [infos["per_agent"][str((i + r) % A)] for i in range(A)],
            "episode_rewards": [infos["episode_rewards"][(i + r) % A] for i in range(A)],
            "time_averaged_game_stats": {key: float.fromhex(v) for key, v in ta["time_averaged_game_stats"].items()}}


def _hex(x):
    return None if x is None else float(x).hex()


def _policy_summaries_equal(got: list, want: list, where: str) -> None:
    assert len(got) == len(want), where
    for p, (g, w) in enumerate(zip(got, want)):
        assert (g["agent_count"], g["action_timeouts"]) == (w["agent_count"], w["action_timeouts"]), (where, p)
        # key order (sorted, summary.py:100) and every bit
        assert [[k, float(v).hex()] for k, v in g["avg_agent_metrics"].items()] == w["avg_agent_metrics"], (where, p)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_summarize_episodes_is_the_references_summary(case):
    episodes = [episode_inputs(case, k) for k in range(len(case["assignments"]))]
    got = summarize_episodes(episodes, case["assignments"], case["num_policies"])
    want = case["summary"]
    assert got["episodes"] == want["episodes"] == len(episodes)
    _policy_summaries_equal(got["policy_summaries"], want["policy_summaries"], case["name"])
    assert {str(i): [_hex(x) for x in row] for i, row in got["per_episode_per_policy_avg_rewards"].items()} == want["per_episode_per_policy_avg_rewards"]
    for key in ("avg_game_stats", "avg_time_averaged_game_stats"):
        assert {k: float(v).hex() for k, v in got[key].items()} == want[key], (case["name"], key)


def test_fixture_covers_the_edge_cases():
    rows = [row for c in CASES for row in c["summary"]["per_episode_per_policy_avg_rewards"].values()]
    assert any(x is None for row in rows for x in row)                                  # a policy without agents in an episode
    assert any(p["agent_count"] == 0 and p["avg_agent_metrics"] == [] for c in CASES for p in c["summary"]["policy_summaries"])
    assert any(len({tuple(a) for a in c["assignments"]}) > 1 for c in CASES)             # assignments differ between episodes
    late = next(c for c in CASES if c["name"] == "chains_late_policy")                   # agents only after the first episode
    assert late["summary"]["policy_summaries"][2]["agent_count"] == 0 and any(2 in a for a in late["assignments"][1:])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_summarize_policy_totals_reproduces_policy_summaries(case):
    """Totals formed on the host in the device's order (records in agent order, one chunk in list order) give the reference's
    policy_summaries bit for bit.  The inputs hold integer-valued stats only: every partial sum is an integer below 2^53, so
    any order of summation is exact and the device's order agrees with the reference's (episodes outermost)."""
    P = case["num_policies"]
    episodes = [episode_inputs(case, k) for k in range(len(case["assignments"]))]
    values = [v for e in episodes for d in e["per_agent"] for v in d.values()]
    assert values and all(float(v) == int(v) and abs(v) < 2 ** 40 for v in values)
    names = sorted({k for e in episodes for d in e["per_agent"] for k in d})
    recs = [policy_record(e["per_agent"], e["episode_rewards"], asg, P) for e, asg in zip(episodes, case["assignments"])]
    tot = PolicyHostTotals(names, P)
    tot.add_step(recs)
    got = summarize_policy_totals(tot.as_dict(), case["assignments"][0])
    assert got["episodes"] == case["summary"]["episodes"]
    _policy_summaries_equal(got["policy_summaries"], case["summary"]["policy_summaries"], case["name"])
    assert [p["agent_episodes"] for p in got["policy_summaries"]] == [sum(list(a).count(p) for a in case["assignments"]) for p in range(P)]
    # two windows (one episode each, then the rest) summed in order: the same
    if len(recs) > 1:
        w1, w2 = PolicyHostTotals(names, P), PolicyHostTotals(names, P)
        w1.add_step(recs[:1]); w2.add_step(recs[1:])
        both = summarize_policy_totals([w1.as_dict(), w2.as_dict()], case["assignments"][0])
        _policy_summaries_equal(both["policy_summaries"], case["summary"]["policy_summaries"], case["name"] + " windows")
    # the per-episode reward rows are the records' (summary.py:81-94)
    assert {str(i): [_hex(x) for x in r["avg_rewards"]] for i, r in enumerate(recs)} == case["summary"]["per_episode_per_policy_avg_rewards"]
