"""Batched PufferEnv-shaped environment over the MI355X step engine.

Mirrors the surface PufferLib drives on the reference's ``MettaGridPufferEnv``
(/root/reference/python/src/mettagrid/envs/mettagrid_puffer_env.py): ``reset(seed) -> (obs, infos)``,
``step(actions) -> (obs, rewards, terminals, truncations, infos)``, the same action encodings (1-D combined index or
``[N, 2]`` primary/vibe columns, :305-394), the same dtypes (:59-63) and lazy auto-reset (an env whose agents are all
terminal or all truncated is restarted at the START of the next ``step`` call, then stepped, :299-302) — for
``num_agents = E * A`` agents at once, with every buffer resident in HBM.  pufferlib itself is not imported.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .compiler import Program
from .engine import BatchedMettaGrid


def split_action_names(action_names: list) -> tuple:
    """PolicyEnvInterface._split_action_names (python/src/mettagrid/policy/policy_env_interface.py:110-119)."""
    primary = [a for a in action_names if not a.startswith("change_vibe_")]
    vibe = [a for a in action_names if a.startswith("change_vibe_")]
    return primary, vibe


def decode_actions(actions, num_primary: int, vibe_action_ids, xp=np):
    """Action decoding rules of MettaGridPufferEnv.step (:305-381).  Returns (core_actions, vibe_actions or None).
    ``xp`` is numpy or torch (the arrays stay on their device)."""
    num_vibe = len(vibe_action_ids)
    if num_primary <= 0:
        raise ValueError("Environment must expose at least one non-vibe action")
    a = actions
    vibe = None
    if a.ndim == 2:
        if a.shape[1] == 1:
            core = a[:, 0]
        elif a.shape[1] == 2:
            core = a[:, 0]
            if num_vibe <= 0:
                raise ValueError("Received 2D actions with vibe column, but environment has no configured vibe action space")
            raw = a[:, 1].to(xp.int64) if xp is not np else a[:, 1].astype(np.int64)
            if bool((raw < 0).any()):
                raise ValueError(f"Vibe actions must be non-negative, got min={int(raw.min())}")
            if bool((raw >= num_vibe).any()):
                raise ValueError(f"Vibe action indices out of range [0,{num_vibe}), min={int(raw.min())} max={int(raw.max())}")
            vibe = vibe_action_ids[raw]
        else:
            raise ValueError(f"Expected step actions shape [num_agents] or [num_agents,2], got {tuple(a.shape)}")
    elif a.ndim == 1:
        a64 = a.to(xp.int64) if xp is not np else a.astype(np.int64)
        if bool((a64 < 0).any()):
            raise ValueError(f"Actions must be non-negative, got min={int(a64.min())}")
        core = a64
        enc = a64 >= num_primary
        if bool(enc.any()):
            if num_vibe <= 0:
                raise ValueError("Received encoded vibe actions, but environment has no configured vibe action space")
            max_valid = num_primary + num_primary * num_vibe
            if bool((a64 >= max_valid).any()):
                raise ValueError(f"Action indices out of range [0, {max_valid}), min={int(a64.min())} max={int(a64.max())}")
            off = a64 - num_primary
            core = xp.where(enc, off // num_vibe, a64)
            vibe = xp.where(enc, vibe_action_ids[(off % num_vibe) * enc], 0 * a64)
    else:
        raise ValueError(f"Expected step actions shape [num_agents] or [num_agents,2], got {tuple(a.shape)}")
    c64 = core.to(xp.int64) if xp is not np else core.astype(np.int64)
    if bool((c64 < 0).any()) or bool((c64 >= num_primary).any()):
        raise ValueError(f"Core actions out of range [0,{num_primary}), min={int(c64.min())} max={int(c64.max())}")
    return core, vibe


def split_supervisor_actions_inplace(teacher_actions, vibe_actions, *, num_primary_actions: int, vibe_action_ids_by_index) -> None:
    """Supervisor (teacher) labels in split-action id space -> primary labels + the simulator's vibe stream, in place:
    ``split_supervisor_actions_inplace`` of the reference (python/src/mettagrid/policy/supervisor_actions.py:8-40).  Labels
    in [0, P) are primary actions; labels in [P, P + V) are vibe v = label - P and fill ``vibe_actions`` with that vibe's
    engine action id, 0 elsewhere.  numpy arrays or torch tensors (torch: the range check is one device->host read)."""
    is_np = isinstance(teacher_actions, np.ndarray)
    t64 = teacher_actions.astype(np.int64) if is_np else teacher_actions.long()
    n_vibe = int(len(vibe_action_ids_by_index))
    max_id = num_primary_actions + n_vibe - 1
    invalid = (t64 < 0) | (t64 > max_id)
    if bool(invalid.any()):
        bad = int(np.flatnonzero(invalid)[0]) if is_np else int(invalid.nonzero()[0, 0])
        raise ValueError(f"Supervisor produced invalid action id {int(teacher_actions[bad])} for agent {bad}")
    primary = t64 < num_primary_actions
    if is_np:
        vibe_actions.fill(0)
        idx = t64[~primary] - num_primary_actions
        vibe_actions[~primary] = np.asarray(vibe_action_ids_by_index)[idx].astype(vibe_actions.dtype)
    else:
        import torch
        ids = torch.as_tensor(vibe_action_ids_by_index, device=teacher_actions.device).long()
        idx = (t64 - num_primary_actions).clamp(min=0)
        vibe_actions.copy_(torch.where(primary, torch.zeros_like(t64), ids[idx * (~primary)] if n_vibe else torch.zeros_like(t64))
                           .to(vibe_actions.dtype))


def decode_actions_unchecked(a, num_primary: int, vibe_action_ids):
    """decode_actions for torch tensors without the range checks (each of them is a device->host read)."""
    import torch
    num_vibe = len(vibe_action_ids)
    if a.ndim == 2:
        if a.shape[1] == 1:
            return a[:, 0], None
        return a[:, 0], vibe_action_ids[a[:, 1].to(torch.int64)]
    a64 = a.to(torch.int64)
    if num_vibe <= 0:
        return a64, None
    enc = a64 >= num_primary
    off = (a64 - num_primary).clamp(min=0)
    core = torch.where(enc, off // num_vibe, a64)
    vibe = torch.where(enc, vibe_action_ids[(off % num_vibe) * enc], torch.zeros_like(a64))
    return core, vibe


STEP_INFO_ATTRIBUTES = ("seed", "map_w", "map_h", "steps", "max_steps")


def parse_step_info_keys(step_info_keys) -> tuple:
    """``MettaGridPufferEnv._configure_step_info_keys`` (mettagrid_puffer_env.py:132-183), host-only: the keys sorted into
    (game keys [(raw key, game stat name)], attribute keys [(raw key, attribute)], agent keys [name]), duplicates dropped in
    first-seen order, with the reference's ValueErrors.  ``env_`` in front of a game / attributes / team key is dropped;
    ``team/<t>/<s>`` is the game stat ``<t>/<s>``.  An attribute the reference does not know raises its ValueError
    (:257-260) here, where the reference raises it from the first payload it builds."""
    game, attrs, agent = [], [], []
    for key in step_info_keys or ():
        key_str = str(key)
        if key_str.startswith("agent/"):
            agent_key = key_str[len("agent/"):]
            if not agent_key:
                raise ValueError("step_info_keys contains invalid entry 'agent/' (missing key suffix)")
            agent.append(agent_key)
            continue
        raw = key_str[len("env_"):] if key_str.startswith("env_") else key_str
        if raw.startswith("game/"):
            stat_key = raw[len("game/"):]
            if not stat_key:
                raise ValueError("step_info_keys contains invalid entry 'game/' (missing key suffix)")
            game.append((raw, stat_key))
            continue
        if raw.startswith("attributes/"):
            attr_key = raw[len("attributes/"):]
            if not attr_key:
                raise ValueError("step_info_keys contains invalid entry 'attributes/' (missing key suffix)")
            if attr_key not in STEP_INFO_ATTRIBUTES:
                raise ValueError(f"Unsupported step_info_keys attribute {raw!r}. Supported: seed, map_w, map_h, steps, max_steps.")
            attrs.append((raw, attr_key))
            continue
        if raw.startswith("team/"):
            remainder = raw[len("team/"):]
            slash = remainder.find("/")
            if slash <= 0:
                raise ValueError(f"step_info_keys entry {key_str!r}: expected 'team/{{team}}/{{stat}}'")
            stat_key = remainder[slash + 1:]
            if not stat_key:
                raise ValueError(f"step_info_keys entry {key_str!r}: missing stat key after team name")
            game.append((raw, f"{remainder[:slash]}/{stat_key}"))
            continue
        raise ValueError(f"Unsupported step_info_keys entry {key_str!r}; "
                         "expected 'game/...', 'attributes/...', 'team/...', or 'agent/...'.")
    return tuple(dict.fromkeys(game)), tuple(dict.fromkeys(attrs)), tuple(dict.fromkeys(agent))


class StepInfo:
    """What ``MettaGridBatchedEnv.step`` puts under ``infos["step_info"]`` when ``step_info_keys`` are set: the last step's
    values of the chosen keys for ALL envs, on the device and ordered on the caller's stream like the observations.

    ``game`` f32 [E, KG] / ``game_exists`` u8 [E, KG]: column k is ``game_columns[k]`` (a game stat name, or
    ``"attributes/steps"``); ``agent`` f32 [E*A, KA] / ``agent_exists`` u8 [E*A, KA]: column k is ``agent_keys[k]``.  A key
    whose exists flag is 0 is one the reference's payload omits.  ``game_keys`` / ``attribute_keys`` / ``agent_keys`` are the
    parsed key lists (``parse_step_info_keys``); ``constants`` holds the attributes that never change (map_w, map_h,
    max_steps; seed: ``seeds`` [E])."""

    def __init__(self, env: "MettaGridBatchedEnv") -> None:
        self._env = env
        self.game_keys, self.attribute_keys, self.agent_keys = env._si_keys
        self.game_columns = env._si_game_columns
        # (keys that are all host constants need no readout: no tensors)
        self.game, self.game_exists, self.agent, self.agent_exists = env.engine.step_stats or (None,) * 4
        words = env.prog.words
        self.constants = {"map_w": float(words[4]), "map_h": float(words[3]), "max_steps": float(words[11])}
        self.seeds = env._seeds()

    def payload(self, env: int) -> dict:
        """The dict ``MettaGridPufferEnv._build_step_info_payload`` (mettagrid_puffer_env.py:230-282) would have returned for
        env ``env`` after this step, without the episode-end infos it starts from: ``{raw key: float}`` for the game and
        attribute keys that exist and ``_per_agent_infos`` ``{agent index: {key: float}}`` when agent keys are set.
        Synchronises with the device: for tests and debugging."""
        A = self._env.prog.num_agents
        if self.game is not None:
            g, ge = self.game[env].cpu().numpy(), self.game_exists[env].cpu().numpy()
        col = {name: k for k, name in enumerate(self.game_columns)}
        out = {}
        for raw, stat in self.game_keys:
            if ge[col[stat]]:
                out[raw] = float(g[col[stat]])
        for raw, attr in self.attribute_keys:
            if attr == "seed":
                out[raw] = float(self.seeds[env])
            elif attr == "steps":
                out[raw] = float(g[col["attributes/steps"]])
            else:
                out[raw] = self.constants[attr]
        if self.agent_keys:
            a = self.agent[env * A:(env + 1) * A].cpu().numpy()
            ae = self.agent_exists[env * A:(env + 1) * A].cpu().numpy()
            out["_per_agent_infos"] = {i: {k: float(a[i, c]) for c, k in enumerate(self.agent_keys) if ae[i, c]} for i in range(A)}
        return out


class MettaGridBatchedEnv:
    """E envs x A agents behind the PufferEnv call pattern.

    Three sources of maps for new episodes (exactly one is given):

    * ``map_pool`` (uint16 [M, H, W], class index + 1): the maps are uploaded to the GPU once and finished envs restart
      ON THE DEVICE (``mgx_set_map_pool`` / ``mgx_set_auto_reset``): no host round trip per step, episode ``k`` of env
      ``e`` plays pool map ``(e + k * pool_stride) mod M``.  ``desync=True`` ends every env's FIRST episode early at a
      step drawn like the reference's ``EarlyResetHandler`` (envs/early_reset_handler.py:6-22:
      ``default_rng(seed).integers(1, max_steps + 1)``), so that envs sharing ``max_steps`` do not all restart on the
      same step.
    * ``map_fn(env_index, episode_index) -> uint16 class map [H, W]``: maps built on the host once per episode, as in the
      reference (simulator.py:83); the done test then costs a device->host read per step.
    * ``map_gen`` (a ``mapgen.RandomMapSpec``, a ``mapgen.MapGenSpec`` or a ``mapgen.MazeGenSpec``; ``mapgen.spec_from_config``
      makes any of them from the dict of a reference map builder config): a fresh map per episode like ``map_fn``, generated ON
      THE DEVICE at restart like ``map_pool`` (``mgx_set_map_generator`` / ``mgx_set_map_scene_generator`` /
      ``mgx_set_map_maze_generator``): the reference's RandomMapBuilder, or its MapGen with a Random instance scene (the arena's
      map builder) or with a Maze instance scene and a Random child, seeded ``base[e] + k`` for episode ``k`` of env ``e``
      (simulator.py:403-409), ``base[e] = (map_seed + e * map_seed_stride) mod 2**32``.  ``map_seed_stride``
      defaults to 2**16, so the seed ranges of two envs do not overlap before an env has played 2**16 episodes (for up to
      2**16 envs; beyond that the bases wrap).  ``desync`` as for ``map_pool``.  ``engine.map_seeds()`` / episode-log records
      (``base[env] + episode``) name the seed of a played map and ``engine.generate_maps`` rebuilds it.

    Engine seeds: ``seed_fn(base, env, episode)`` (default: the seed given to ``reset`` plus the env index, constant
    across auto-resets like the reference's ``_current_seed``).

    With device buffers the returned tensors are ordered on the caller's current torch stream (no host synchronisation).
    ``validate_actions``: ``True`` — the reference's range checks on the action tensor are made by the decode kernel on the
    device and a bad id raises the reference's ValueError from a LATER ``step`` / ``check_actions()`` call (no host read on the
    good path; 1-D int32 tensors — other layouts take the host-synchronous path); ``"strict"`` — checked on the host before
    the step runs, as the reference does (a device->host read per check); ``False`` — no check.

    ``infos`` (the last element of what ``step`` returns): the reference's wrapper returns, from the step that ends an episode
    on, the dict StatsTracker.on_episode_end built (stats_tracker.py:26-76: ``game``, ``agent``, ``per_agent``, ``attributes``
    ...).  Here dozens of the E envs finish in any one step; their stats are reduced on the device before the restart wipes
    them (``episode_stats=True``: include/mgx.h "Episode-end statistics") and ``step`` returns the batch aggregate of the
    episodes that finished since the last non-empty ``infos``: ``{"episodes": n, "game": {key: mean over the episodes that
    hold the key}, "agent": {key: mean of the per-episode infos["agent"] values}, "game_count" / "agent_count",
    "episode_return": {mean, min, max}, "episode_length": {...}, "terminated": n, "attributes": {...}}`` — every
    ``stats_interval`` steps a snapshot is requested and the one requested before is returned if its copy has landed (no
    host synchronisation: the aggregate trails the step that produced it by ``stats_interval`` steps), ``{}`` otherwise.
    ``episode_infos()`` returns the finished episodes one by one in the reference's shape from a bounded device log
    (``episode_log`` records; ``log_per_agent`` adds ``per_agent``).

    ``step_info_keys``: the reference's per-step payload (mettagrid_puffer_env.py:81, 132-183, 230-282) — ``game/<stat>``,
    ``team/<team>/<stat>``, ``attributes/seed|map_w|map_h|steps|max_steps`` (each with an optional ``env_`` prefix),
    ``agent/<stat>``, ``agent/reward_step``, ``agent/reward_episode``.  A kernel behind every step gathers the chosen values of
    all envs and agents on the device (``BatchedMettaGrid.set_step_stats``; device buffers only) and ``step`` returns them as
    ``infos["step_info"]``, a ``StepInfo``: the tensors, the key lists and ``payload(env)``, the reference's dict for one env.
    A step that ends an episode reports that episode's final values, the next step those of the restarted episode.  ``reset``
    returns no payload (the tensors are written by steps).  Without keys ``infos`` is what it is without this argument.

    ``time_averaged_stats``: the reference's TimeAveragedStatsHandler (simulator/time_averaged_stats.py:17-41) for every env,
    accumulated on the device (``BatchedMettaGrid.set_time_averages``; needs ``episode_stats``).  The aggregate ``infos`` gets
    ``"time_averaged_game": {key: sum of the episodes' averages / episodes}`` — the rule of multi_episode/summary.py:72-74:
    divided by the number of episodes, not by the number holding the key — and ``"time_averaged_count"`` (and ``"time_averaged_partial": n`` when n of the window's episodes were partial: they are in
    ``infos["episodes"]`` but in neither of the two); every
    ``episode_infos()`` entry gets ``"time_averaged_game_stats"`` (and ``"time_averaged_partial": True`` when the accumulation did
    not cover the whole episode); ``save_state`` / ``load_state`` carry the accumulators in ``EnvState.extra["time_avg"]``.  Off: ``infos`` and ``episode_infos()`` are what they are without this argument.

    ``policy_assignments`` (``[A]``, every env alike, or ``[E][A]``) and ``num_policies`` (default: the largest index + 1): which
    policy drives which agent row, for evaluating several policies in one game; every finished episode's agent stats and
    returns are reduced per policy on the device (``BatchedMettaGrid.set_policy_stats``; needs ``episode_stats``), in the
    arithmetic of multi_episode/summary.py:38-130.  The aggregate ``infos`` gets ``"policy"``: per policy ``episodes`` (those in
    which it had an agent), ``agent_episodes``, ``avg_reward`` ({mean, min, max} of the per-episode average reward, or None),
    ``agent_sum`` {key: f64 sum over its agents and the episodes} and ``agent_count`` {key: episodes}; every ``episode_infos()``
    entry gets ``"assignments"`` (the row the episode ended under) and ``"policy_avg_rewards"`` ([P] floats or None: the
    reference's per_episode_per_policy_avg_rewards row).  ``policy_ids`` (int64 [E * A]) and ``policy_rows(p)`` route
    observations and actions; ``set_policy_assignments(envs, rows)`` rematches slots between episodes.  The table belongs to
    the slots: ``save_state`` / ``load_state`` do not move it.  Off: ``infos`` and ``episode_infos()`` are unchanged.

    ``map_weights`` (with ``map_pool``; f64 [M], or ``"uniform"``: equal weights, the distribution of the reference's map cache,
    simulator/map_cache.py:207-215): auto-resets draw the next pool map with probability proportional to the weights instead of
    rotating (``BatchedMettaGrid.set_pool_sampling``; the draw is ``pool_sampling.draws(weights, map_sample_seed,
    map_env_offset, [env], [episode])``, reproducible bit for bit); ``set_map_weights(w)`` replaces them between steps without
    waiting for the device — the curriculum's half of the loop.  The first episode's maps stay ``arange(E) % M``.
    ``map_env_offset``: the global index of env 0 when several wrappers share one batch (``dist.env_shard(...).start``).
    ``map_stats`` (needs ``episode_stats`` and ``map_pool``): per-map episode statistics reduced on the device; the aggregate
    ``infos`` gets ``"per_map"``, a list with one dict per pool map, and ``"unattributed"``, one more such dict for the episodes
    without a pool index (every slot's first): each with ``episodes``, ``terminated``, ``length_sum``, ``return_sum`` (fixed point, 2**-20), ``return_min``, ``return_max`` over the
    same window, and with ``map_labels`` (one label per pool map) ``"per_label_rewards": {label: return_sum / episodes}`` over the
    window's episodes of that label's maps (stats_tracker.py:59-60 for a batch).  Off: ``infos`` is unchanged.
    ``global_state`` (device buffers): every env's whole state as a token row on the device — what a centralised critic
    reads (``BatchedMettaGrid.set_global_state``; format: ``mettagrid_amd/global_state.py``).  ``env.global_state`` is
    ``(tokens uint32 [E, TG], counts uint32 [E], agent_start int32 [E, A])``: device tensors that ``step`` updates in place,
    and ``reset`` / ``load_state`` through ``write_global_state``.  ``global_state_exclude``: classes left out (cell or type
    names such as ``"wall"``, class ids); ``global_state_tokens``: TG (default: the engine's bound).  With device restarts a
    finished env's row shows its final state, like its observations, and the restarted env after its first step.
    ``token_bag`` (device buffers): ``True`` or ``"float32"`` / ``"bfloat16"`` — the token-bag features of every observation
    row (``BatchedMettaGrid.token_bag``; ``mettagrid_amd/token_bag.py``), what a token policy's ``TokenBagEmbedding`` reads.
    ``env.token_bag`` is ``(bag [E*A, 32 + C], counts int32 [E*A])``: device tensors written behind every ``step``'s
    observations and by ``reset`` / ``load_state``, in place, ordered on the caller's stream like the other returned tensors.
    With device restarts a finished env's rows follow its observation rows.
    ``render_envs`` (device buffers) and ``render_scale`` (tile size s, default 8): ``env.frames`` is a device tensor uint8
    [n, H * s, W * s, 3] with one RGB frame per listed env (``BatchedMettaGrid.render_rgb`` with the atlas of
    ``render.default_tiles``; ``engine.set_render_tiles`` replaces it), kept current in place behind every ``step``, ``reset``
    and ``load_state`` and ordered on the caller's stream like ``token_bag``.  With device restarts a finished env's frame
    shows its final state, and the restarted env appears after its first step, as its observations do.  ``render()`` works
    without it.
    """

    def __init__(self, prog: Program, num_envs: int, map_fn: Optional[Callable[[int, int], np.ndarray]] = None,
                 seed_fn: Optional[Callable[[int, int, int], int]] = None, device: int = 0, seed: int = 0,
                 buffers: str = "device", map_pool: Optional[np.ndarray] = None, pool_stride: int = 1,
                 desync: bool = False, validate_actions: bool = True, episode_stats: bool = True, stats_interval: int = 1,
                 episode_log: int = 0, log_per_agent: bool = False, specialize="auto", replay_envs=None,
                 replay_dir: Optional[str] = None, replay_words_per_env: Optional[int] = None, replay_interval: int = 64,
                 replay_capacity_groups: Optional[dict] = None, map_gen=None, map_seed: int = 0,
                 map_seed_stride: int = 1 << 16, step_info_keys=None, time_averaged_stats: bool = False,
                 policy_assignments=None, num_policies: Optional[int] = None, map_weights=None, map_sample_seed: int = 0,
                 map_stats: bool = False, map_labels=None, map_env_offset: int = 0, global_state: bool = False,
                 global_state_exclude=(), global_state_tokens: Optional[int] = None, token_bag=False,
                 render_envs=None, render_scale: int = 8) -> None:
        if global_state and buffers != "device":
            raise ValueError("global_state needs device buffers")
        if token_bag not in (False, True, "float32", "bfloat16"):
            raise ValueError('token_bag: False, True, "float32" or "bfloat16"')
        if token_bag and buffers != "device":
            raise ValueError("token_bag needs device buffers")
        self._tb_dtype = None if not token_bag else "bfloat16" if token_bag == "bfloat16" else "float32"
        self.token_bag = None             # (bag, counts) once reset() has made the engine
        self.render_scale = int(render_scale)
        if not 1 <= self.render_scale <= 32:
            raise ValueError("render_scale must be in [1, 32]")
        self.render_envs = None           # int32 list of the envs whose frames are kept current, or None
        self.frames = None                # uint8 [n, H * s, W * s, 3] once reset() has made the engine
        if render_envs is not None:
            from .engine import env_list
            if buffers != "device":
                raise ValueError("render_envs needs device buffers")
            self.render_envs = env_list(list(render_envs), num_envs, "render_envs")
        self._gs_on, self._gs_exclude, self._gs_tokens = bool(global_state), tuple(global_state_exclude), global_state_tokens
        self.global_state = None          # (tokens, counts, agent_start) once reset() has made the engine
        if map_weights is not None and map_pool is None:
            raise ValueError("map_weights needs map_pool")
        if map_stats and (not episode_stats or map_pool is None):
            raise ValueError("map_stats needs episode_stats and map_pool")
        if map_labels is not None and not map_stats:
            raise ValueError("map_labels needs map_stats")
        if map_labels is not None and len(map_labels) != len(map_pool):
            raise ValueError("map_labels: one label per pool map")
        if isinstance(map_weights, str):
            if map_weights != "uniform":
                raise ValueError('map_weights: an array of one weight per pool map, or "uniform"')
            map_weights = np.ones(len(map_pool), np.float64)
        if map_weights is not None:
            from .pool_sampling import quantise
            map_weights = np.array(map_weights, dtype=np.float64)
            if map_weights.shape != (len(map_pool),):
                raise ValueError("map_weights: one weight per pool map")
            quantise(map_weights)   # (refuses what the engine would refuse at reset())
        self.map_weights = map_weights
        self.map_sample_seed, self.map_env_offset = int(map_sample_seed), int(map_env_offset)
        self.map_stats = bool(map_stats)
        self.map_labels = None if map_labels is None else list(map_labels)
        if time_averaged_stats and not episode_stats:
            raise ValueError("time_averaged_stats needs episode_stats")
        if policy_assignments is not None and not episode_stats:
            raise ValueError("policy_assignments needs episode_stats")
        if policy_assignments is None and num_policies is not None:
            raise ValueError("num_policies needs policy_assignments")
        self._policy_table = None         # host copy of the engine's assignment table, u8 [E][A]
        if policy_assignments is not None:
            a = np.asarray(policy_assignments)
            if a.ndim == 1:
                a = np.broadcast_to(a, (num_envs, len(a)))
            if a.shape != (num_envs, prog.num_agents) or a.dtype.kind not in "iub" or (a < 0).any() or (a > 255).any():
                raise ValueError(f"policy_assignments: integers in [0, 255] of shape [{prog.num_agents}] or [{num_envs}][{prog.num_agents}]")
            self._policy_table = np.array(a, dtype=np.uint8)
            self.num_policies = int(a.max()) + 1 if num_policies is None else int(num_policies)
        self._policy_ids = None
        self._pending_infos: list = []    # episodes drained by set_policy_assignments, returned by the next episode_infos()
        self.time_averaged_stats = bool(time_averaged_stats)
        self._si_keys = parse_step_info_keys(step_info_keys)
        # the game columns of the readout: the distinct stat names, then the step counter when an attribute key asks for it
        self._si_game_columns = list(dict.fromkeys(stat for _, stat in self._si_keys[0]))
        if any(attr == "steps" for _, attr in self._si_keys[1]):
            self._si_game_columns.append("attributes/steps")
        self._si_on = any(self._si_keys)
        if self._si_on and buffers != "device":
            raise ValueError("step_info_keys needs device buffers")
        if (map_fn is not None) + (map_pool is not None) + (map_gen is not None) != 1:
            raise ValueError("give exactly one of map_fn, map_pool and map_gen")
        self.map_gen = map_gen
        self.map_seed, self.map_seed_stride = int(map_seed), int(map_seed_stride)
        self._device_restarts = map_fn is None    # finished envs restart on the device (pool or generator): no done read per step
        self.prog = prog
        self.E = num_envs
        self.map_fn = map_fn
        self.map_pool = None if map_pool is None else np.ascontiguousarray(map_pool, dtype=np.uint16)
        self.pool_stride = pool_stride
        self.desync = desync
        self.validate_actions = validate_actions
        self._default_seed_fn = seed_fn is None
        self.seed_fn = seed_fn or (lambda base, env, episode: (base + env) & 0xFFFFFFFF)
        self._seed = seed
        self._device = device
        self._kind = buffers
        self.action_names, self.vibe_action_names = split_action_names(prog.action_names)
        self.num_agents = num_envs * prog.num_agents
        self.episode = np.zeros(num_envs, np.int64)
        self._eng: Optional[BatchedMettaGrid] = None
        self._vibe_ids = None
        self.supervisor = None          # object with step_batch(raw_observations, teacher_actions), see set_supervisor
        self.teacher_actions = None
        self.episode_stats = episode_stats
        self.stats_interval = max(1, int(stats_interval))
        self.episode_log = int(episode_log)
        self.log_per_agent = log_per_agent
        self.specialize = specialize      # BatchedMettaGrid(specialize=...): run-time code objects for this program (jit.py)
        self._steps = 0
        # replays of watched envs (BatchedMettaGrid.set_replay; mettagrid_amd/replay.py)
        self.replay_envs = [int(e) for e in (replay_envs or [])]
        self.replay_dir = replay_dir
        self.replay_words_per_env = replay_words_per_env
        self.replay_interval = max(1, int(replay_interval))
        self.replay_capacity_groups = replay_capacity_groups
        self.replay_paths: dict = {}      # (env, episode index of that env) -> file written
        self.replays_overflowed = 0       # drains that found a watched env's log full (that episode is not written)
        if self.replay_envs and buffers != "device":
            raise ValueError("replay_envs needs device buffers")
        if self.replay_envs and not replay_dir:
            raise ValueError("replay_envs needs replay_dir")

    def set_supervisor(self, supervisor) -> None:
        """Supervisor-policy path of MettaGridPufferEnv (mettagrid_puffer_env.py:399-426): after every step
        ``supervisor.step_batch(observations, teacher_actions)`` fills ``teacher_actions`` (split-action id space) and the
        vibe labels are routed into the engine's vibe stream for the next step."""
        self.supervisor = supervisor

    def disable_supervisor(self) -> None:
        self.supervisor = None

    def _compute_supervisor_actions(self) -> None:
        eng = self.engine
        if self.teacher_actions is None:
            if self._kind == "device":
                import torch
                self.teacher_actions = torch.zeros(self.num_agents, dtype=torch.int32, device=eng.obs.device)
            else:
                self.teacher_actions = np.zeros(self.num_agents, np.int32)
        self.supervisor.step_batch(eng.obs, self.teacher_actions)
        split_supervisor_actions_inplace(self.teacher_actions, eng.vibe_actions, num_primary_actions=len(self.action_names),
                                         vibe_action_ids_by_index=self._vibe_ids if self._kind != "device" else self._vibe_ids)

    # spaces (shapes only; gymnasium is not a dependency)
    @property
    def single_observation_shape(self):
        return (self.prog.num_tokens, 3)

    @property
    def single_action_n(self) -> int:
        return len(self.action_names)

    @property
    def transport_action_n(self) -> int:
        n, v = len(self.action_names), len(self.vibe_action_names)
        return n * (v + 1) if v else n

    def _maps(self, envs) -> np.ndarray:
        H = int(self.prog.words[3]), int(self.prog.words[4])
        out = np.zeros((self.E,) + H, np.uint16)
        for e in envs:
            out[e] = self.map_fn(int(e), int(self.episode[e]))
        return out

    def _seeds(self) -> np.ndarray:
        if self._default_seed_fn:   # (base + env) mod 2^32 for every env at once
            return ((np.int64(self._seed) + np.arange(self.E, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)
        return np.array([self.seed_fn(self._seed, e, int(self.episode[e])) for e in range(self.E)], dtype=np.uint32)

    def map_seed_bases(self) -> np.ndarray:
        """``map_gen``: the map seed base of every env, uint32 [E]."""
        return ((self.map_seed + np.arange(self.E, dtype=np.int64) * self.map_seed_stride) & 0xFFFFFFFF).astype(np.uint32)

    def early_end_steps(self) -> np.ndarray:
        """EarlyResetHandler.on_episode_start for every env: one draw from a generator seeded with the env's seed."""
        ms = int(self.prog.words[11])   # MGX_H_MAX_STEPS
        if ms <= 0:
            return np.zeros(self.E, np.uint32)
        from .early_reset import first_integers
        return first_integers(self._seeds(), ms)

    def reset(self, seed: Optional[int] = None):
        if seed is not None:
            self._seed = seed
        if self._eng is not None:
            self._eng.close()
        self.episode[:] = 0
        if self.map_pool is not None:
            M = self.map_pool.shape[0]
            first = self.map_pool[np.arange(self.E) % M]
            self._eng = BatchedMettaGrid(self.prog, first, self._seeds(), device=self._device, buffers=self._kind,
                                         specialize=self.specialize)
            self._eng.set_map_pool(self.map_pool)
            self._eng.set_auto_reset(True, self.pool_stride, self.early_end_steps() if self.desync else None)
            if self.map_weights is not None:
                self._eng.set_pool_sampling(self.map_weights, self.map_sample_seed, self.map_env_offset)
        elif self.map_gen is not None:
            from .mapgen import generated_class_maps
            # capacities are sized from the create maps, and every map of a recipe holds the same cells: one host-built map
            one = generated_class_maps(self.map_gen, self.prog, [int(self.map_seed_bases()[0])])
            self._eng = BatchedMettaGrid(self.prog, np.broadcast_to(one, (self.E,) + one.shape[1:]), self._seeds(), device=self._device,
                                         buffers=self._kind, specialize=self.specialize)
            self._eng.set_map_generator(self.map_gen, self.map_seed_bases())
            self._eng.reset_envs_generated(np.ones(self.E, np.uint8))
            self._eng.set_auto_reset(True, 1, self.early_end_steps() if self.desync else None)
        else:
            self._eng = BatchedMettaGrid(self.prog, self._maps(range(self.E)), self._seeds(), device=self._device,
                                         buffers=self._kind, specialize=self.specialize)
        if self.episode_stats:
            self._eng.set_episode_stats(True, self.episode_log, self.log_per_agent)
            if self.time_averaged_stats:
                self._eng.set_time_averages(True, self.episode_log)
            if self._policy_table is not None:
                self._eng.set_policy_stats(True, self.num_policies, self._policy_table, self.episode_log)
            if self.map_stats:
                self._eng.set_map_stats(True)
        self._policy_ids = None
        self._pending_infos = []
        self._steps = 0
        if self._si_on and (self._si_game_columns or self._si_keys[2]):
            self._eng.set_step_stats(self._si_game_columns, self._si_keys[2])
        self._step_info = StepInfo(self) if self._si_on else None   # (one object: the engine rewrites its tensors every step)
        self.global_state = self._eng.set_global_state(self._gs_tokens, self._gs_exclude) if self._gs_on else None
        self.token_bag = None
        if self._tb_dtype is not None:
            import torch
            rows, dev = self.E * self.prog.num_agents, self._eng.obs.device
            bag = torch.empty((rows, 32 + len(self.prog.feature_norms)), dtype=getattr(torch, self._tb_dtype), device=dev)
            counts = torch.empty((rows,), dtype=torch.int32, device=dev)
            self._eng.wait_for_caller()   # (the allocator may hand out memory the caller's stream still uses)
            self.token_bag = self._eng.token_bag(bag, counts)
        self.frames = None
        if self.render_envs is not None:
            self._eng.set_render_tiles(scale=self.render_scale)
            self._eng.wait_for_caller()   # (as above: the frames may be memory the caller's stream still uses)
            self.frames = self._eng.render_rgb(self.render_envs)
        if self.replay_envs:
            from .replay import ReplayAssembler
            import os
            os.makedirs(self.replay_dir, exist_ok=True)
            self._eng.set_replay(self.replay_envs, words_per_env=self.replay_words_per_env)
            self._assemblers = [ReplayAssembler(self.prog, capacity_groups=self.replay_capacity_groups) for _ in self.replay_envs]
            self._replay_count = [0] * len(self.replay_envs)          # episode index of the next replay of each watched env
            self._replay_unnumbered = [False] * len(self.replay_envs)  # an episode was lost to overflow: indices unknown from there on
            self._replay_steps = 0
            self.replay_paths = {}
        ids = [self.prog.action_names.index(n) for n in self.vibe_action_names]
        self._vibe_ids_host = np.asarray(ids, dtype=np.int32)
        if self._kind == "device":
            import torch
            self._vibe_ids = torch.tensor(ids, dtype=torch.int64, device=self._eng.obs.device)
            self._eng.caller_waits()
        else:
            self._vibe_ids = np.asarray(ids, dtype=np.int64)
        return self._eng.obs, {}

    @property
    def engine(self) -> BatchedMettaGrid:
        if self._eng is None:
            raise RuntimeError("Simulation is closed")
        return self._eng

    def _done_envs(self) -> np.ndarray:
        eng = self.engine
        A = self.prog.num_agents
        if self._kind == "device":
            eng.sync()
            term = eng.terminals.view(self.E, A).all(dim=1) | eng.truncations.view(self.E, A).all(dim=1)
            return term.cpu().numpy()
        return eng.terminals.reshape(self.E, A).all(1) | eng.truncations.reshape(self.E, A).all(1)

    # ---- infos ----
    def _infos_from_totals(self, tot: Optional[dict]) -> dict:
        """Batch aggregate of the finished episodes in the vocabulary of StatsTracker.on_episode_end (stats_tracker.py:26-76)."""
        if not tot or tot["episodes"] == 0:
            return {}
        n = tot["episodes"]
        words = self.prog.words
        return {"episodes": n,
                "game": {k: v / tot["game_count"][k] for k, v in tot["game_sum"].items()},
                "agent": {k: v / tot["agent_count"][k] for k, v in tot["agent_sum"].items()},
                "game_count": tot["game_count"], "agent_count": tot["agent_count"],
                "episode_return": {"mean": tot["return_sum"] / n, "min": tot["return_min"], "max": tot["return_max"]},
                "episode_length": {"mean": tot["length_sum"] / n, "min": tot["length_min"], "max": tot["length_max"]},
                "terminated": int(tot["terminated"]),
                "attributes": {"map_w": int(words[4]), "map_h": int(words[3]), "max_steps": int(words[11]), "seed": self._seed}}

    def _with_time_averages(self, infos: dict, ta: Optional[dict]) -> dict:
        """The batch's time-averaged game stats beside the aggregate (summary.py:72-74: sum over episodes / episodes).  The two
        snapshots are requested together, so they cover the same episodes; partial episodes are in neither value."""
        if ta and ta["episodes"] > 0:
            infos = dict(infos, time_averaged_game={k: v / ta["episodes"] for k, v in ta["sum"].items()},
                         time_averaged_count=ta["count"])
        if ta and ta["partial"] > 0:   # counted in infos["episodes"], in neither time_averaged_game nor its divisor
            infos = dict(infos, time_averaged_partial=ta["partial"])
        return infos

    @staticmethod
    def _with_policies(infos: dict, ps: Optional[dict]) -> dict:
        """The batch's per-policy totals beside the aggregate (requested with it, so over the same episodes)."""
        if not ps or ps["episodes"] == 0:
            return infos
        pol = [{"episodes": p["episodes"], "agent_episodes": p["agent_episodes"],
                "avg_reward": {"mean": p["avg_reward_sum"] / p["episodes"], "min": p["avg_reward_min"], "max": p["avg_reward_max"]}
                if p["episodes"] else None,
                "agent_sum": p["agent_sum"], "agent_count": p["agent_count"]} for p in ps["policies"]]
        return dict(infos, policy=pol)

    def _with_maps(self, infos: dict, ms: Optional[list]) -> dict:
        """The window's per-map table beside the aggregate (requested with it, so over the same episodes)."""
        if not ms or not any(m["episodes"] for m in ms):
            return infos
        infos = dict(infos, per_map=ms[:-1], unattributed=ms[-1])
        if self.map_labels is not None:
            tot: dict = {}
            for label, m in zip(self.map_labels, ms):
                if m["episodes"]:
                    t = tot.setdefault(label, [0.0, 0])
                    t[0] += m["return_sum"]
                    t[1] += m["episodes"]
            infos["per_label_rewards"] = {label: t[0] / t[1] for label, t in tot.items()}
        return infos

    def _step_infos(self) -> dict:
        if not self.episode_stats:
            return {}
        eng = self.engine
        self._steps += 1
        ta_on, ps_on, ms_on = self.time_averaged_stats, self._policy_table is not None, self.map_stats
        if not self._device_restarts or self._kind != "device":   # these paths synchronise with the device every step anyway
            if self._steps % self.stats_interval != 0:
                return {}
            out = self._infos_from_totals(eng.drain_episode_stats())
            if ta_on:
                out = self._with_time_averages(out, eng.drain_time_averages())
            if ps_on:
                out = self._with_policies(out, eng.drain_policy_stats())
            return self._with_maps(out, eng.drain_map_stats()) if ms_on else out
        out = {}
        if self._steps % self.stats_interval == 0:
            if ta_on or ps_on or ms_on:
                # the snapshots are requested back to back and fetched together: the copy of the one requested last lands
                # last, so once it is there the others are too (no wait), and until then none is taken
                ms = eng.fetch_map_stats(wait=False) if ms_on else None
                landed = ms is not None
                ps = eng.fetch_policy_stats(wait=landed) if ps_on and (landed or not ms_on) else None
                landed = landed or ps is not None
                ta = eng.fetch_time_averages(wait=landed) if ta_on and (landed or not (ms_on or ps_on)) else None
                if landed or ta is not None:
                    out = self._infos_from_totals(eng.fetch_episode_stats(wait=True))
                    if ta_on:
                        out = self._with_time_averages(out, ta)
                    out = self._with_policies(out, ps)
                    out = self._with_maps(out, ms)
            else:
                out = self._infos_from_totals(eng.fetch_episode_stats(wait=False))   # the snapshot requested one interval ago
            eng.request_episode_stats()
            if ta_on:
                eng.request_time_averages()
            if ps_on:
                eng.request_policy_stats()
            if ms_on:
                eng.request_map_stats()
        return out

    def set_map_weights(self, weights) -> None:
        """New sampling weights (``map_weights``) from the next step's restarts on; does not wait for the device."""
        if self.map_weights is None:
            raise ValueError("no map_weights")
        w = np.array(weights, dtype=np.float64)
        self.engine.set_pool_weights(w)
        self.map_weights = w

    # ---- policies (policy_assignments) ----
    @property
    def policy_ids(self):
        """The policy index of every agent row, int64 [E * A] where the buffers are (a device tensor with device buffers)."""
        if self._policy_table is None:
            raise ValueError("no policy_assignments")
        if self._policy_ids is None:
            flat = self._policy_table.reshape(-1).astype(np.int64)
            if self._kind == "device":
                import torch
                self._policy_ids = torch.from_numpy(flat).to(self.engine.obs.device)
            else:
                self._policy_ids = flat
        return self._policy_ids

    def policy_rows(self, p: int):
        """The agent rows policy ``p`` drives, ascending: the index of an ``index_select`` on observations or actions."""
        ids = self.policy_ids
        if self._kind == "device":
            import torch
            return torch.nonzero(ids == int(p)).reshape(-1)
        return np.nonzero(ids == int(p))[0]

    def set_policy_assignments(self, envs, rows) -> None:
        """Replace the assignment rows of ``envs`` (``rows``: ``[A]`` or ``[n][A]``): episodes that end from now on are
        attributed by them.  Synchronises; the episodes logged so far are kept, with the rows they ended under, for the next
        ``episode_infos()``."""
        if self._policy_table is None:
            raise ValueError("no policy_assignments")
        from .engine import env_list
        lst = env_list(envs, self.E, "set_policy_assignments", unique=True)
        if self.episode_log > 0:
            self._pending_infos += self._drain_episode_infos()
        self.engine.set_policy_assignments(lst, rows)
        r = np.asarray(rows)
        self._policy_table[lst] = r if r.ndim == 2 else np.broadcast_to(r, (len(lst), len(r)))
        self._policy_ids = None

    def action_sampler(self, seed: int = 0):
        """A ``sampling.ActionSampler`` for this env's joint actions: ``E * A`` rows of
        ``transport_action_n`` logits on the engine's device.  Its ``actions`` tensor (1-D int32, the shape of the engine's
        action buffer) is what ``step`` takes on its one-kernel path: ``env.step(s.sample(logits)[0])``.  Needs device
        buffers and a ``reset()``."""
        if self._kind != "device":
            raise ValueError("action_sampler needs device buffers")
        from .sampling import ActionSampler
        eng = self.engine
        return ActionSampler(self.E * self.prog.num_agents, self.transport_action_n, seed=seed, device=eng.obs.device)

    def check_actions(self, wait: bool = True) -> None:
        """Raise the reference's ValueError for a joint action id the device-side decode found out of range
        (mettagrid_puffer_env.py:336-360).  ``step`` calls this with ``wait=False`` (no synchronisation: an error surfaces at
        a later step, the offending ids having been played as invalid actions); call it with ``wait=True`` for certainty."""
        flags, row, value = self.engine.poll_action_errors(wait)
        if flags & 1:
            raise ValueError(f"Actions must be non-negative, got {value} for agent {row}")
        if flags & 2:
            n, v = len(self.action_names), len(self.vibe_action_names)
            raise ValueError(f"Action indices out of range [0, {n + n * v if v else n}), got {value} for agent {row}")

    def flush_replays(self) -> list:
        """Drain the watched envs' logs (synchronises with the device) and write one file per episode that finished in them:
        ``<replay_dir>/env<e>_ep<k>.json.z``, k = the env's episode index as the episode log counts it.  Returns the paths
        written by this call.  ``step`` calls it when a watched env finishes where it has the done flags on the host anyway
        (host map source); with a map pool the step never reads them (auto-reset is on the device), so there the logs are
        drained every ``replay_interval`` steps — a device synchronisation each time — and by ``episode_infos()`` / ``close()``.
        An episode lost to a full log (``replays_overflowed``) leaves no END marker, so the env's later episodes can no longer
        be numbered: their files are named ``env<e>_unnumbered<n>.json.z`` and are not attached to ``episode_infos()``."""
        if not self.replay_envs or self._eng is None:
            return []
        from .fmt import K
        from .replay import write_replay
        import os
        words, flags = self.engine.drain_replay()
        out = []
        for k, env in enumerate(self.replay_envs):
            for ep in self._assemblers[k].feed(words[k]):
                n = self._replay_count[k]
                if not self._replay_unnumbered[k]:
                    ep["infos"]["attributes"]["seed"] = int(self.seed_fn(self._seed, env, n))
                if self._replay_unnumbered[k]:
                    path = os.path.join(self.replay_dir, f"env{env}_unnumbered{n}.json.z")
                else:
                    path = os.path.join(self.replay_dir, f"env{env}_ep{n}.json.z")
                    self.replay_paths[(env, n)] = path
                write_replay(ep, path)
                self._replay_count[k] += 1
                out.append(path)
            if flags[k] & K.RPL_ENV_OVERFLOW:   # (a drain clears this bit: one lost episode is counted once)
                self.replays_overflowed += 1
            if flags[k] & (K.RPL_ENV_OVERFLOW | K.RPL_ENV_MUTED):   # (behind the episodes that were complete before it)
                self._replay_unnumbered[k] = True
        return out

    def episode_infos(self) -> list:
        """The episodes that finished since the last call, one dict each in the reference's shape (stats_tracker.py:26-76):
        ``game``, ``agent``, ``per_agent`` (with ``log_per_agent``), ``episode_rewards``, ``attributes`` (seed, map_w, map_h,
        steps, max_steps) + ``env`` / ``episode`` / ``map_index``.  Needs ``episode_log`` > 0; synchronises with the device."""
        out = self._pending_infos + self._drain_episode_infos()
        self._pending_infos = []
        return out

    def _drain_episode_infos(self) -> list:
        self.flush_replays()
        recs, dropped = self.engine.drain_episode_log()
        ta = None
        if self.time_averaged_stats:
            # the two logs have the same capacity, fill at the same finish points and are drained together: joined by position
            # (an env can finish several episodes between two drains, and without a pool every record says episode 0)
            ta = self.engine.drain_time_average_log()[0]
            if len(ta) != len(recs) or any((t["env"], t["steps"]) != (r["env"], r["steps"]) for t, r in zip(ta, recs)):
                raise RuntimeError("episode_infos: the episode log and the time-average log do not hold the same episodes")
        ps = None
        if self._policy_table is not None:   # joined by position, as the time-average log
            ps = self.engine.drain_policy_log()[0]
            if len(ps) != len(recs) or any((t["env"], t["steps"]) != (r["env"], r["steps"]) for t, r in zip(ps, recs)):
                raise RuntimeError("episode_infos: the episode log and the policy log do not hold the same episodes")
        words = self.prog.words
        out = []
        for k, r in enumerate(recs):
            info = {"game": r["game"], "agent": r["agent"], "episode_rewards": r["episode_rewards"],
                    "attributes": {"seed": r["seed"], "map_w": int(words[4]), "map_h": int(words[3]), "steps": r["steps"],
                                   "max_steps": int(words[11])},
                    "env": r["env"], "episode": r["episode"], "map_index": r["map_index"]}
            if "per_agent" in r:
                info["per_agent"] = {str(i): dct for i, dct in enumerate(r["per_agent"])}
            if ta is not None:
                info["time_averaged_game_stats"] = ta[k]["time_averaged_game_stats"]
                if ta[k]["partial"]:
                    info["time_averaged_partial"] = True
            if ps is not None:
                info["assignments"] = [int(x) for x in self._policy_table[r["env"]]]
                info["policy_avg_rewards"] = ps[k]["avg_rewards"]
            if (r["env"], r["episode"]) in self.replay_paths:
                info["replay_path"] = self.replay_paths[(r["env"], r["episode"])]
            out.append(info)
        self.episodes_dropped = dropped
        return out

    def step(self, actions):
        eng = self.engine
        if not self._device_restarts:  # host map source: the done test needs the flags on the host
            done = self._done_envs()
            if done.any():  # lazy auto-reset at the start of the next step (mettagrid_puffer_env.py:299-302)
                idx = np.nonzero(done)[0]
                if self.episode_stats:
                    eng.record_episodes(done)
                if self.replay_envs and any(done[e] for e in self.replay_envs):
                    self.flush_replays()
                self.episode[idx] += 1
                eng.reset_envs(done, self._maps(idx), self._seeds())
                # (no write_global_state: the step below rewrites every row)
        if self._kind == "device":
            import torch
            a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions), device=eng.obs.device)
            if self.supervisor is None and self.validate_actions != "strict" and a.ndim == 1 and a.dtype == torch.int32 and a.is_contiguous():
                # one kernel on the engine's stream instead of a dozen elementwise torch kernels; it also makes the reference's
                # range checks (mettagrid_puffer_env.py:336-360) and raises a flag the host reads without synchronising
                if tuple(a.shape) != tuple(eng.actions.shape):
                    raise ValueError(f"Expected {tuple(eng.actions.shape)} actions, got {tuple(a.shape)}")
                if self.validate_actions:
                    self.check_actions(wait=False)      # a bad id of an EARLIER step whose kernel has run by now
                eng.wait_for_caller()
                eng.set_joint_actions(a, len(self.action_names), self._vibe_ids_host)
            else:
                if self.validate_actions:
                    core, vibe = decode_actions(a, len(self.action_names), self._vibe_ids, xp=torch)
                else:
                    core, vibe = decode_actions_unchecked(a, len(self.action_names), self._vibe_ids)
                    if self.supervisor is not None and vibe is not None and a.ndim == 1:
                        # the reference only overwrites the vibe stream when some action of the batch carries a vibe
                        # (:361-381); decided on the device, no host read
                        vibe = torch.where((a >= len(self.action_names)).any(), vibe, eng.vibe_actions.to(vibe.dtype))
                if tuple(core.shape) != tuple(eng.actions.shape):
                    raise ValueError(f"Expected {tuple(eng.actions.shape)} core actions, got {tuple(core.shape)}")
                eng.actions.copy_(core.to(torch.int32))
                if vibe is not None:
                    eng.vibe_actions.copy_(vibe.to(torch.int32))
                elif self.supervisor is None:   # with a supervisor the teacher's vibe labels of the last step stay
                    eng.vibe_actions.zero_()    # (mettagrid_puffer_env.py:389-391)
                eng.wait_for_caller()   # the engine's kernels read the actions written on the caller's stream ...
            eng.step()
            if self.token_bag is not None:
                eng.token_bag(*self.token_bag)
            if self.frames is not None:
                eng.render_rgb(self.render_envs, self.frames)
            eng.caller_waits()      # ... and whatever the caller enqueues next sees this step's results
            if self.supervisor is not None:
                self._compute_supervisor_actions()
        else:
            a = np.asarray(actions)
            core, vibe = decode_actions(a, len(self.action_names), self._vibe_ids, xp=np)
            if core.shape != eng.actions.shape:
                raise ValueError(f"Expected {eng.actions.shape} core actions, got {core.shape}")
            np.copyto(eng.actions, core.astype(np.int32))
            if vibe is not None:
                np.copyto(eng.vibe_actions, vibe.astype(np.int32))
            elif self.supervisor is None:       # mettagrid_puffer_env.py:389-391
                eng.vibe_actions.fill(0)
            eng.step()
            if self.supervisor is not None:
                self._compute_supervisor_actions()
        infos = self._step_infos()
        if self._si_on:
            infos = dict(infos, step_info=self._step_info)
        if self.replay_envs and self._device_restarts:
            self._replay_steps += 1
            if self._replay_steps % self.replay_interval == 0:
                self.flush_replays()
        return eng.obs, eng.rewards, eng.terminals, eng.truncations, infos

    # ---- saving and restoring envs' state (BatchedMettaGrid.save_envs / load_envs) ----
    def save_state(self, envs=None):
        """The state of ``envs`` (default: all) as an ``engine.EnvState``; with ``map_fn`` it also carries the envs' host-side
        episode counters (which pick the next episode's map and seed)."""
        from .engine import env_list
        lst = env_list(envs, self.E, "save_state")
        st = self.engine.save_envs(lst)
        if not self._device_restarts:
            st.extra["episode"] = self.episode[lst].copy()
        if self.time_averaged_stats:   # not part of the engine's record: a resumed episode continues its average
            # one uint32 array [n][2 * NG + seen words + 1] (f64 sums as word pairs, seen bits, steps): survives EnvState.to_dict
            t = self.engine.time_average_state(lst)
            st.extra["time_avg"] = np.concatenate([t["sum"].view(np.uint32).reshape(len(lst), -1), t["seen"], t["steps"][:, None]], axis=1)
        return st

    def load_state(self, state, envs=None) -> None:
        """Put ``state`` into ``envs`` (default: the slots it was saved from); they continue their saved episodes."""
        from .engine import env_list
        lst = env_list(state.envs if envs is None else envs, self.E, "load_state", unique=True)
        self.engine.load_envs(state, lst)
        if self.time_averaged_stats and "time_avg" in state.extra:   # (without them the episode ends flagged partial)
            t = np.ascontiguousarray(state.extra["time_avg"], dtype=np.uint32)
            ng = len(self.prog.game_stat_names)
            self.engine.put_time_average_state(lst, {"sum": np.ascontiguousarray(t[:, :2 * ng]).view(np.float64).reshape(len(lst), ng),
                                                     "seen": t[:, 2 * ng:-1], "steps": t[:, -1]})
        if not self._device_restarts and "episode" in state.extra:
            self.episode[lst] = np.asarray(state.extra["episode"], dtype=np.int64)
        if self._gs_on:   # the rows are derived state: rebuilt from what was loaded
            self.engine.write_global_state(lst)
            self.engine.caller_waits()
        if self.token_bag is not None:   # ... and so are the bags of the loaded observation rows
            self.engine.token_bag(*self.token_bag)
            self.engine.caller_waits()
        if self.frames is not None:      # ... and the frames of the watched envs
            self.engine.render_rgb(self.render_envs, self.frames)
            self.engine.caller_waits()

    # ---- looking at an env (mettagrid_amd/render.py) ----
    @property
    def render_mode(self) -> str:
        """``"ansi"``, as the reference's MettaGridPufferEnv (envs/mettagrid_puffer_env.py:505-508)."""
        return "ansi"

    def render(self, env: int = 0, mode: str = "ansi", symbols=None):
        """Env ``env`` as the reference's text frame (``mode="ansi"``, mettagrid_puffer_env.py:510-524; ``symbols``: the
        overrides the reference reads from ``game.render.symbols``) or as a host uint8 array [H * s, W * s, 3]
        (``mode="rgb_array"``, s = ``render_scale``, the atlas the engine holds or else the default one)."""
        from . import render
        eng = self.engine
        if mode == "ansi":
            return render.ansi(eng.render_cells([int(env)])[0], render.class_type_names(self.prog), symbols)
        if mode != "rgb_array":
            raise ValueError('render: mode must be "ansi" or "rgb_array"')
        if getattr(eng, "render_tiles", None) is None:
            eng.set_render_tiles(scale=self.render_scale)
        eng.wait_for_caller()   # (the new frame may be memory the caller's stream still uses)
        frame = eng.render_rgb([int(env)])
        eng.sync()
        return frame[0].cpu().numpy()

    def close(self) -> None:
        if self._eng is not None:
            self.flush_replays()
            self._eng.close()
            self._eng = None


class MettaGridParallelEnv:
    """PettingZoo ``ParallelEnv`` call pattern over ONE env of the engine — the surface of the reference's
    ``MettaGridPettingZooEnv`` (python/src/mettagrid/envs/pettingzoo_env.py:22-230): integer agent ids, ``reset(seed) ->
    (obs dict, info dict)``, ``step({agent: action}) -> (obs, rewards, terminations, truncations, infos)`` as dicts keyed by
    agent id, finished agents dropped from ``agents``, one shared observation / action space for all agents.  pettingzoo and
    gymnasium themselves are not imported: spaces are described by shape / size."""

    def __init__(self, env_cfg, map, seed: int = 0, device: int = 0, global_state: bool = False,  # noqa: A002 - reference argument name
                 global_state_exclude=(), global_state_tokens: Optional[int] = None, render_mode: Optional[str] = None,
                 render_scale: int = 8, render_symbols=None) -> None:
        """``global_state=True``: ``state()`` returns the env's global state row (``mettagrid_amd/global_state.py``) instead of
        the reference's zero vector; the engine then runs on device buffers and the dicts hold host copies.
        ``render_mode``: what ``render()`` returns — None: nothing, ``"ansi"``: the reference's text frame (``render_symbols``:
        symbol overrides), ``"rgb_array"``: a uint8 array [H * s, W * s, 3] with s = ``render_scale``."""
        from .engine import MettaGrid
        if render_mode not in (None, "ansi", "rgb_array"):
            raise ValueError('render_mode: None, "ansi" or "rgb_array"')
        if not 1 <= int(render_scale) <= 32:
            raise ValueError("render_scale must be in [1, 32]")
        self.render_mode, self._render_scale, self._render_symbols = render_mode, int(render_scale), render_symbols
        self._gs_on = bool(global_state)

        def make(s):
            sim = MettaGrid(env_cfg, map, s, device=device, buffers="device" if self._gs_on else "host")
            if self._gs_on:
                sim._b.set_global_state(global_state_tokens, global_state_exclude, agent_start=False)
            return sim
        self._make = make
        self._seed = seed
        self._sim = self._make(seed)
        names = self._sim.prog.action_names
        self._action_indices = list(range(len(names)))      # PolicyEnvInterface.action_names -> engine action ids
        self.possible_agents = list(range(self._sim._num_agents))
        self.agents = list(self.possible_agents)
        self.observation_shape = (self._sim.prog.num_tokens, 3)

    def reset(self, seed: Optional[int] = None, options=None):
        if seed is not None:
            self._seed = seed
        self._sim._b.close()
        self._sim = self._make(self._seed)
        self.agents = list(self.possible_agents)
        obs = self._host(self._sim.observations())
        return {a: obs[a] for a in self.agents}, {a: {} for a in self.agents}

    def _host(self, x):
        """A bound buffer as a numpy array (device buffers: a host copy behind the engine's stream)."""
        if isinstance(x, np.ndarray):
            return x
        self._sim._b.sync()
        return x.cpu().numpy()

    def step(self, actions: dict):
        sim = self._sim
        arr = sim.actions() if not self._gs_on else np.zeros(len(self.possible_agents), np.int32)
        for a in self.agents:
            if a in actions:
                idx = int(np.asarray(actions[a], dtype=np.int32).reshape(()).item())
                if idx < 0 or idx >= len(self._action_indices):
                    raise ValueError(f"Action index {idx} out of range for PettingZoo action space.")
                arr[a] = self._action_indices[idx]
        if self._gs_on:   # device buffers: the agents that sent nothing keep their previous action, as in the host array
            import torch
            sent = np.zeros(len(arr), np.bool_)
            sent[[a for a in self.agents if a in actions]] = True
            dev = sim.actions().device
            sim.actions().copy_(torch.where(torch.as_tensor(sent, device=dev), torch.as_tensor(arr, device=dev), sim.actions()))
            torch.cuda.synchronize(dev)
        sim.step()
        obs, rew, term, trunc = (self._host(x) for x in (sim.observations(), sim.rewards(), sim.terminals(), sim.truncations()))
        out = ({a: obs[a] for a in self.agents}, {a: float(rew[a]) for a in self.agents}, {a: bool(term[a]) for a in self.agents},
               {a: bool(trunc[a]) for a in self.agents}, {a: {} for a in self.agents})
        self.agents = [a for a in self.agents if not (out[2][a] or out[3][a])]
        return out

    def observation_space_shape(self, agent: int):
        return self.observation_shape

    def action_space_n(self, agent: int) -> int:
        return len(self._action_indices)

    def state(self) -> np.ndarray:
        """Default: the reference's stub, a zero vector of the flattened observation size (pettingzoo_env.py:178-190).  With
        ``global_state=True``: the env's global state row as u8 [TG][4] = (row, col, feature, value), 0xFF behind the last
        token (``mettagrid_amd/global_state.py``)."""
        if self._gs_on:
            return self._host(self._sim._b.global_state[0][0]).view(np.uint8).reshape(-1, 4).copy()
        return np.zeros(len(self.possible_agents) * int(np.prod(self.observation_shape)), np.uint8)

    @property
    def max_num_agents(self) -> int:
        return len(self.possible_agents)

    @property
    def max_steps(self) -> int:
        return self._sim.max_steps

    def render(self):
        """None without a ``render_mode``; the text frame for ``"ansi"``; the RGB frame (host array) for ``"rgb_array"``."""
        if self.render_mode is None:
            return None
        from . import render
        b = self._sim._b
        if self.render_mode == "ansi":
            return render.ansi(b.render_cells([0])[0], render.class_type_names(b.prog), self._render_symbols)
        if getattr(b, "render_tiles", None) is None:
            b.set_render_tiles(scale=self._render_scale)
        b.wait_for_caller()   # (the new frame may be memory the caller's stream still uses)
        frame = b.render_rgb([0])
        b.sync()
        return frame[0].cpu().numpy()

    def close(self) -> None:
        if self._sim is not None:
            self._sim._b.close()
            self._sim = None
