"""Host only: mettagrid_amd.summary.summarize_episodes is the reference's build_multi_episode_rollout_summaries for one mission
(python/src/mettagrid/simulator/multi_episode/summary.py:38-130).  The expectations below are that function's arithmetic
written out by hand: every sum in episode (then agent) order, divided once at the end."""
import numpy as np

from mettagrid_amd.summary import summarize_episodes


def _episodes():
    """Three episodes of three agents.  "b" is missing from the second episode's dicts, "late" only exists in the third."""
    return [
        {"game": {"a": 1.0, "b": 0.1}, "time_averaged_game_stats": {"a": 0.5, "b": 0.1}, "episode_rewards": np.float32([1.0, 2.0, 4.0]),
         "per_agent": {"0": {"z": 1.0, "m": 0.1}, "1": {"m": 0.2}, "2": {"z": 3.0, "m": 0.3}}},
        {"game": {"a": 2.0}, "time_averaged_game_stats": {"a": 0.25}, "episode_rewards": np.float32([0.5, 0.25, 0.125]),
         "per_agent": {"0": {"m": 0.4}, "1": {"m": 0.5, "k": 7.0}, "2": {"m": 0.6}}},
        {"game": {"a": 4.0, "b": 0.2, "late": 3.0}, "time_averaged_game_stats": {"a": 0.125, "b": 0.7, "late": 0.3},
         "episode_rewards": np.float32([3.0, 0.0, -1.0]),
         "per_agent": {"0": {"z": 5.0}, "1": {}, "2": {"m": 0.7}}},
    ]


def _bits(x) -> bytes:
    return np.float64(x).tobytes()


def test_two_policies_three_episodes():
    s = summarize_episodes(_episodes(), [0, 1, 0], 2)
    assert s["episodes"] == 3
    # a key missing from one episode is still divided by ALL episodes (summary.py:69-74)
    assert s["avg_game_stats"] == {"a": ((1.0 + 2.0) + 4.0) / 3, "b": (0.1 + 0.2) / 3, "late": 3.0 / 3}
    want_ta = {"a": ((0.5 + 0.25) + 0.125) / 3, "b": (0.1 + 0.7) / 3, "late": 0.3 / 3}
    assert s["avg_time_averaged_game_stats"].keys() == want_ta.keys()
    for k, v in want_ta.items():
        assert _bits(s["avg_time_averaged_game_stats"][k]) == _bits(v), k
    p0, p1 = s["policy_summaries"]
    assert p0["agent_count"] == 2 and p1["agent_count"] == 1 and p0["action_timeouts"] == p1["action_timeouts"] == 0
    # policy 0 = agents 0 and 2: sums in episode order, inside an episode in agent order; divided by the agent count
    m0 = ((((0.1 + 0.3) + 0.4) + 0.6) + 0.7) / 2
    z0 = ((1.0 + 3.0) + 5.0) / 2
    assert list(p0["avg_agent_metrics"]) == ["m", "z"]           # sorted keys (summary.py:100)
    assert _bits(p0["avg_agent_metrics"]["m"]) == _bits(m0) and _bits(p0["avg_agent_metrics"]["z"]) == _bits(z0)
    assert list(p1["avg_agent_metrics"]) == ["k", "m"]
    assert _bits(p1["avg_agent_metrics"]["m"]) == _bits((0.2 + 0.5) / 1) and p1["avg_agent_metrics"]["k"] == 7.0
    assert s["per_episode_per_policy_avg_rewards"] == {0: [(1.0 + 4.0) / 2, 2.0], 1: [(0.5 + 0.125) / 2, 0.25], 2: [(3.0 + -1.0) / 2, 0.0]}


def test_policy_without_agents_gives_none_and_no_metrics():
    s = summarize_episodes(_episodes(), [0, 0, 0], 2)
    p0, p1 = s["policy_summaries"]
    assert p0["agent_count"] == 3 and p1 == {"agent_count": 0, "avg_agent_metrics": {}, "action_timeouts": 0}
    assert s["per_episode_per_policy_avg_rewards"] == {0: [((1.0 + 2.0) + 4.0) / 3, None], 1: [((0.5 + 0.25) + 0.125) / 3, None],
                                                       2: [((3.0 + 0.0) + -1.0) / 3, None]}
    assert list(p0["avg_agent_metrics"]) == ["k", "m", "z"]
    assert _bits(p0["avg_agent_metrics"]["m"]) == _bits((((((0.1 + 0.2) + 0.3) + 0.4) + 0.5) + 0.6 + 0.7) / 3)


def test_no_episodes_and_episodes_without_time_averages():
    s = summarize_episodes([], [0, 1], 2)
    assert s["episodes"] == 0 and s["avg_game_stats"] == {} and s["avg_time_averaged_game_stats"] == {}
    assert s["per_episode_per_policy_avg_rewards"] == {} and [p["agent_count"] for p in s["policy_summaries"]] == [1, 1]
    eps = [{k: v for k, v in e.items() if k != "time_averaged_game_stats"} for e in _episodes()]
    assert summarize_episodes(eps, [0, 1, 0], 2)["avg_time_averaged_game_stats"] == {}
    # per-episode assignment lists: the counts come from the first episode's (summary.py:48)
    s = summarize_episodes(_episodes(), [[0, 1, 0], [1, 1, 1], [0, 0, 0]], 2)
    assert [p["agent_count"] for p in s["policy_summaries"]] == [2, 1]
    assert s["per_episode_per_policy_avg_rewards"][1] == [None, ((0.5 + 0.25) + 0.125) / 3]
