"""BUILD-CONTAINER ONLY — golden output of the reference's own ``build_multi_episode_rollout_summaries``.

    python tests/golden/make_policy_summary_fixture.py

Builds ``EpisodeRolloutResult`` lists (python/src/mettagrid/simulator/multi_episode/rollout.py:10-22) from the committed
fixtures of the reference's own episodes — infos_chains.json / infos_navigation.json (``per_agent``, ``game``,
``episode_rewards``; tests/golden/make_infos_fixture.py) and time_avg_chains.json / time_avg_navigation.json
(tests/golden/make_time_avg_fixture.py) — and runs the REFERENCE's summary over them
(python/src/mettagrid/simulator/multi_episode/summary.py:38-130).  A case is one mission: a scenario, a number of policies and
one assignment list per episode; episode k of a case is the fixture's episode with its agents rotated by ``rotate[k]`` rows
(agent i plays what agent i + r played), so that the episodes of a case differ.  The cases cover a policy without any agent
(``None`` rewards, no metrics), a policy without agents in the FIRST episode only (agent_count 0 although it has sums),
assignments that differ between episodes, and one policy per agent.
Output: tests/golden/policy_summary.json — the cases (data only) and the reference's output, floats as ``float.hex()``.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_fixtures as mrf  # noqa: E402

CASES = [
    {"name": "chains_two_policies", "scenario": "chains", "num_policies": 2, "rotate": [0], "assignments": [[0, 1, 0, 1, 0, 1]]},
    {"name": "chains_policy_without_agents", "scenario": "chains", "num_policies": 3, "rotate": [0, 2],
     "assignments": [[0, 0, 0, 1, 1, 1], [1, 1, 0, 0, 1, 0]]},
    {"name": "chains_late_policy", "scenario": "chains", "num_policies": 3, "rotate": [0, 1, 3],
     "assignments": [[0, 1, 0, 1, 0, 1], [2, 2, 0, 1, 1, 0], [1, 0, 2, 0, 2, 1]]},
    {"name": "navigation_changing", "scenario": "navigation", "num_policies": 2, "rotate": [0, 1],
     "assignments": [[0, 0, 1, 1], [1, 0, 1, 0]]},
    {"name": "navigation_policy_per_agent", "scenario": "navigation", "num_policies": 5, "rotate": [0, 3, 2],
     "assignments": [[0, 1, 2, 3], [3, 2, 1, 0], [4, 0, 4, 1]]},
]


def episode_inputs(case: dict, k: int) -> dict:
    """Episode k of a case from the committed fixtures: {"game", "per_agent" (a list), "episode_rewards",
    "time_averaged_game_stats"} (tests/test_policy_summary_fixture.py restates these lines)."""
    infos = json.load(open(os.path.join(HERE, f"infos_{case['scenario']}.json")))
    ta = json.load(open(os.path.join(HERE, f"time_avg_{case['scenario']}.json")))
    A, r = len(infos["per_agent"]), case["rotate"][k]
    return {"game": infos["game"], "per_agent": [infos["per_agent"][str((i + r) % A)] for i in range(A)],
            "episode_rewards": [infos["episode_rewards"][(i + r) % A] for i in range(A)],
            "time_averaged_game_stats": {key: float.fromhex(v) for key, v in ta["time_averaged_game_stats"].items()}}


def hexed(x):
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {str(k): hexed(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [hexed(v) for v in x]
    return x


def main() -> None:
    import typing
    import typing_extensions
    typing.TypedDict = typing_extensions.TypedDict   # (Python < 3.12: pydantic takes no typing.TypedDict as a field type)
    mrf.import_reference(shim=False)
    from mettagrid.simulator.multi_episode.rollout import EpisodeRolloutResult, MultiEpisodeRolloutResult
    from mettagrid.simulator.multi_episode.summary import build_multi_episode_rollout_summaries
    out = []
    for case in CASES:
        episodes = []
        for k, asg in enumerate(case["assignments"]):
            e = episode_inputs(case, k)
            episodes.append(EpisodeRolloutResult(assignments=asg, rewards=e["episode_rewards"], action_timeouts=[0] * len(asg),
                                                 stats={"game": e["game"], "agent": e["per_agent"]}, replay_path=None, steps=0, max_steps=0,
                                                 time_averaged_game_stats=e["time_averaged_game_stats"]))
        (s,) = build_multi_episode_rollout_summaries([MultiEpisodeRolloutResult(episodes=episodes)], case["num_policies"])
        d = s.model_dump()
        # key order is part of the result (sorted metric keys, summary.py:100): kept as lists of pairs
        d["policy_summaries"] = [dict(p, avg_agent_metrics=[[k, float(v).hex()] for k, v in p["avg_agent_metrics"].items()])
                                 for p in d["policy_summaries"]]
        out.append(dict(case, summary=hexed(d)))
    p = os.path.join(HERE, "policy_summary.json")
    json.dump(out, open(p, "w"), separators=(",", ":"), sort_keys=True)
    print(p, os.path.getsize(p), "bytes;", len(out), "cases")


if __name__ == "__main__":
    main()
