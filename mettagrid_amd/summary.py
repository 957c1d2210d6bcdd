"""Summary of a batch of finished episodes of one mission — the reference's ``build_multi_episode_rollout_summaries``
(python/src/mettagrid/simulator/multi_episode/summary.py:38-130) over the dicts ``MettaGridBatchedEnv.episode_infos()`` returns.

Host only; every sum is taken in the reference's order (Python floats = f64): game stats and time-averaged game stats over
the episodes in list order, a policy's agent metrics over episodes and, inside an episode, over its agents in agent order."""
from __future__ import annotations

import numpy as np


def _assignments_of(assignments, n_episodes: int) -> list:
    """One policy index per agent, for all episodes (a flat sequence) or per episode (a sequence of sequences)."""
    a = list(assignments)
    if a and np.ndim(a[0]) > 0:
        if len(a) != n_episodes:
            raise ValueError(f"summarize_episodes: {len(a)} assignment lists for {n_episodes} episodes")
        return [[int(p) for p in row] for row in a]
    flat = [int(p) for p in a]
    return [flat] * max(1, n_episodes)


def _agent_dicts(info: dict) -> list:
    """infos["per_agent"] ({"0": {...}, ...}, or a list) in agent order; [] when the log was kept without per-agent rows."""
    pa = info.get("per_agent", [])
    if isinstance(pa, dict):
        return [pa[k] for k in sorted(pa, key=int)]
    return list(pa)


def summarize_episodes(episodes: list, assignments, num_policies: int) -> dict:
    """``episodes``: dicts with ``game``, ``episode_rewards``, optionally ``time_averaged_game_stats`` and ``per_agent``;
    ``assignments``: the policy index of every agent.  Returns ``{"episodes", "avg_game_stats", "avg_time_averaged_game_stats",
    "policy_summaries": [{"agent_count", "avg_agent_metrics", "action_timeouts"}], "per_episode_per_policy_avg_rewards"}``."""
    n = len(episodes)
    assign = _assignments_of(assignments, n)
    policy_counts = np.bincount(np.asarray(assign[0], dtype=np.int64), minlength=num_policies)   # summary.py:48

    summed_game: dict = {}
    summed_ta: dict = {}
    summed_policy = [dict() for _ in range(num_policies)]
    for e, asg in zip(episodes, assign):   # summary.py:54-67
        for key, value in e.get("game", {}).items():
            summed_game[key] = summed_game.get(key, 0.0) + float(value)
        for key, value in e.get("time_averaged_game_stats", {}).items():
            summed_ta[key] = summed_ta.get(key, 0.0) + float(value)
        for agent_id, stats in enumerate(_agent_dicts(e)):
            if agent_id >= len(asg):
                continue
            tgt = summed_policy[asg[agent_id]]
            for key, value in stats.items():
                tgt[key] = tgt.get(key, 0.0) + float(value)

    # divided by the number of episodes, not by the number holding the key (summary.py:69-77)
    avg_game = {k: v / n for k, v in summed_game.items()} if n else {}
    avg_ta = {k: v / n for k, v in summed_ta.items()} if n else {}

    per_episode: dict = {}
    for idx, (e, asg) in enumerate(zip(episodes, assign)):   # summary.py:81-94
        totals = np.zeros(num_policies, dtype=float)
        counts = np.zeros(num_policies, dtype=int)
        for agent_id, reward in enumerate(e.get("episode_rewards", ())):
            if agent_id >= len(asg):
                continue
            totals[asg[agent_id]] += float(reward)
            counts[asg[agent_id]] += 1
        per_episode[idx] = [float(totals[i] / counts[i]) if counts[i] > 0 else None for i in range(num_policies)]

    policies = []
    for p in range(num_policies):   # summary.py:96-118
        count = int(policy_counts[p]) if p < len(policy_counts) else 0
        metrics = {k: v / count for k, v in sorted(summed_policy[p].items())} if count > 0 else {}
        policies.append({"agent_count": count, "avg_agent_metrics": metrics, "action_timeouts": 0})   # (no action timeouts here)

    return {"episodes": n, "policy_summaries": policies, "avg_game_stats": avg_game, "avg_time_averaged_game_stats": avg_ta,
            "per_episode_per_policy_avg_rewards": per_episode}


def summarize_policy_totals(window_totals, assignments_of_first_episode) -> dict:
    """The per-policy half of the summary from the device's totals (``BatchedMettaGrid.policy_totals_dict``: one window's
    dict, or a list of windows' dicts, added in list order) instead of per-agent log rows.

    The reference's own rule is kept (summary.py:48, 96-103): ``agent_count`` = bincount of the FIRST episode's assignments and
    ``avg_agent_metrics[key]`` = the sum over ALL episodes and agents of the policy / that count, keys sorted — not a
    per-episode mean when assignments differ between episodes or there are several episodes.  ``agent_episodes`` (how many
    agent rows the sums run over) is returned beside it, so a caller can form ``sum / agent_episodes``.
    Returns ``{"episodes", "policy_summaries": [{"agent_count", "avg_agent_metrics", "action_timeouts", "agent_episodes"}]}``."""
    windows = [window_totals] if isinstance(window_totals, dict) else list(window_totals)
    num_policies = len(windows[0]["policies"]) if windows else 0
    counts = np.bincount(np.asarray(list(assignments_of_first_episode), dtype=np.int64), minlength=num_policies)   # summary.py:48
    policies = []
    for p in range(num_policies):
        summed: dict = {}
        agent_episodes = 0
        for w in windows:
            for key, value in w["policies"][p]["agent_sum"].items():
                summed[key] = summed.get(key, 0.0) + float(value)
            agent_episodes += int(w["policies"][p]["agent_episodes"])
        count = int(counts[p])
        metrics = {k: v / count for k, v in sorted(summed.items())} if count > 0 else {}   # summary.py:96-103
        policies.append({"agent_count": count, "avg_agent_metrics": metrics, "action_timeouts": 0, "agent_episodes": agent_episodes})
    return {"episodes": sum(int(w["episodes"]) for w in windows), "policy_summaries": policies}
