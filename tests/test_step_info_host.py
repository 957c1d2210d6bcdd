"""Host-only: the step_info_keys grammar of MettaGridPufferEnv._configure_step_info_keys
(python/src/mettagrid/envs/mettagrid_puffer_env.py:132-183) as mettagrid_amd.envs.parse_step_info_keys restates it — every
accepted form, every ValueError of the reference with its text, first-seen order of duplicates — and the resolution of stat
names to the column codes of include/mgx_program.h (a name the program's tables do not hold is MGX_SS_ABSENT)."""
import numpy as np
import pytest

from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv, parse_step_info_keys
from mettagrid_amd.fmt import K


def test_every_accepted_form():
    game, attrs, agent = parse_step_info_keys([
        "game/objects.wall", "env_game/tokens_written", "team/red/ore.amount", "env_team/blue/score",
        "attributes/seed", "attributes/map_w", "attributes/map_h", "env_attributes/steps", "attributes/max_steps",
        "agent/action.move.success", "agent/reward_step", "agent/reward_episode", "agent/env_x"])
    assert game == (("game/objects.wall", "objects.wall"), ("game/tokens_written", "tokens_written"),
                    ("team/red/ore.amount", "red/ore.amount"), ("team/blue/score", "blue/score"))
    assert attrs == (("attributes/seed", "seed"), ("attributes/map_w", "map_w"), ("attributes/map_h", "map_h"),
                     ("attributes/steps", "steps"), ("attributes/max_steps", "max_steps"))
    assert agent == ("action.move.success", "reward_step", "reward_episode", "env_x")


def test_team_stat_keeps_its_later_slashes():
    game, _, _ = parse_step_info_keys(["team/red/a/b"])
    assert game == (("team/red/a/b", "red/a/b"),)


def test_env_prefix_is_not_stripped_from_agent_keys():
    # the reference tests for "agent/" before it strips "env_": "env_agent/x" is no agent key and matches no other form
    with pytest.raises(ValueError) as e:
        parse_step_info_keys(["env_agent/x"])
    assert str(e.value) == ("Unsupported step_info_keys entry 'env_agent/x'; "
                            "expected 'game/...', 'attributes/...', 'team/...', or 'agent/...'.")


def test_none_and_empty_mean_no_keys():
    assert parse_step_info_keys(None) == ((), (), ())
    assert parse_step_info_keys([]) == ((), (), ())


def test_keys_are_taken_through_str():
    class Key:
        def __str__(self):
            return "game/objects.wall"
    assert parse_step_info_keys([Key()])[0] == (("game/objects.wall", "objects.wall"),)


@pytest.mark.parametrize("keys, message", [
    (["agent/"], "step_info_keys contains invalid entry 'agent/' (missing key suffix)"),
    (["game/"], "step_info_keys contains invalid entry 'game/' (missing key suffix)"),
    (["env_game/"], "step_info_keys contains invalid entry 'game/' (missing key suffix)"),
    (["attributes/"], "step_info_keys contains invalid entry 'attributes/' (missing key suffix)"),
    (["team/red"], "step_info_keys entry 'team/red': expected 'team/{team}/{stat}'"),
    (["team//x"], "step_info_keys entry 'team//x': expected 'team/{team}/{stat}'"),
    (["env_team/red"], "step_info_keys entry 'env_team/red': expected 'team/{team}/{stat}'"),
    (["team/red/"], "step_info_keys entry 'team/red/': missing stat key after team name"),
    (["objects.wall"], "Unsupported step_info_keys entry 'objects.wall'; expected 'game/...', 'attributes/...', 'team/...', or 'agent/...'."),
    (["game/ok", "stats/x"], "Unsupported step_info_keys entry 'stats/x'; expected 'game/...', 'attributes/...', 'team/...', or 'agent/...'."),
    # (the reference raises this one from the first payload it builds, mettagrid_puffer_env.py:257-260)
    (["env_attributes/episode"], "Unsupported step_info_keys attribute 'attributes/episode'. Supported: seed, map_w, map_h, steps, max_steps."),
])
def test_every_rejection_of_the_reference(keys, message):
    with pytest.raises(ValueError) as e:
        parse_step_info_keys(keys)
    assert str(e.value) == message


def test_duplicates_keep_first_seen_order():
    game, attrs, agent = parse_step_info_keys([
        "game/b", "agent/y", "game/a", "env_game/b", "agent/x", "attributes/steps", "agent/y", "game/a", "env_attributes/steps",
        "attributes/seed", "team/b/c", "game/b/c"])
    # "env_game/b" repeats ("game/b", "b"); "team/b/c" and "game/b/c" name the same stat under two raw keys: both stay
    assert game == (("game/b", "b"), ("game/a", "a"), ("team/b/c", "b/c"), ("game/b/c", "b/c"))
    assert attrs == (("attributes/steps", "steps"), ("attributes/seed", "seed"))
    assert agent == ("y", "x")


def _prog():
    return compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)


def test_unknown_stat_names_resolve_to_the_absent_code():
    prog = _prog()
    eng = BatchedMettaGrid.__new__(BatchedMettaGrid)   # (the resolution needs the program only: no engine, no GPU)
    eng.prog = prog
    g, a = eng.step_stat_columns(["objects.wall", "no.such.stat", "attributes/steps", "reward_step"],
                                 ["action.move.success", "reward_step", "no.such.stat", "reward_episode", "action.invalid_index.400",
                                  "attributes/steps"])
    assert g.dtype == np.int32 and a.dtype == np.int32
    assert g.tolist() == [prog.game_stat_names.index("objects.wall"), K.SS_ABSENT, K.SS_STEPS, K.SS_ABSENT]
    assert a.tolist() == [prog.agent_stat_names.index("action.move.success"), K.SS_REWARD_STEP, K.SS_ABSENT, K.SS_REWARD_EPISODE,
                          K.SS_ABSENT, K.SS_ABSENT]
    assert (K.SS_ABSENT, K.SS_REWARD_STEP, K.SS_REWARD_EPISODE, K.SS_STEPS) == (-1, -2, -3, -4) and K.SS_MAX_COLUMNS == 64


def test_the_env_sorts_keys_into_columns_and_refuses_host_buffers():
    prog = _prog()
    pool = np.stack([prog.class_map(presets.rung3_map(50))])
    env = MettaGridBatchedEnv(prog, 2, map_pool=pool, step_info_keys=[
        "game/objects.wall", "team/red/x", "env_game/objects.wall", "attributes/steps", "attributes/seed", "agent/reward_step"])
    assert env._si_game_columns == ["objects.wall", "red/x", "attributes/steps"] and env._si_keys[2] == ("reward_step",)
    assert MettaGridBatchedEnv(prog, 2, map_pool=pool, step_info_keys=["attributes/seed"])._si_game_columns == []
    assert not MettaGridBatchedEnv(prog, 2, map_pool=pool)._si_on
    with pytest.raises(ValueError, match="device buffers"):
        MettaGridBatchedEnv(prog, 2, map_pool=pool, buffers="host", step_info_keys=["agent/reward_step"])
    with pytest.raises(ValueError, match="missing key suffix"):
        MettaGridBatchedEnv(prog, 2, map_pool=pool, step_info_keys=["game/"])
