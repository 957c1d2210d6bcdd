"""Saved env state, host side (include/mgx.h mgx_env_state_layout; no GPU): the record layout and format word the planner
gives a program and its create maps, the header constants, and the Python env-list checks that run before any C call."""
import ctypes

import numpy as np
import pytest

import helpers as hp
from mettagrid_amd import engine, presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.fmt import K


def _prog_maps(name: str, seeds=(0, 1)):
    spec_f, map_f, _, _ = hp.scenario(name)
    maps = [map_f(s) for s in seeds]
    prog = hp.compile_scenario(name, spec_f(), *maps[0].shape)
    return prog, np.stack([prog.class_map(m) for m in maps])


def test_layout_record_size_and_alignment():
    prog, cms = _prog_maps("rung3")
    info = engine.env_state_layout(prog, cms)
    A, T = prog.num_agents, prog.num_tokens
    caller = A * T * 3 + A * 4 + 2 * A
    assert info["record_bytes"] % K.ES_ALIGN == 0
    assert info["record_bytes"] >= K.ES_HEADER_BYTES + caller + 624 * 4
    assert info["version"] == K.ES_VERSION and info["n_segments"] > 10 and info["pool_tokens"] > 0


def test_format_is_stable_and_tells_programs_apart():
    p3, m3 = _prog_maps("rung3")
    p4, m4 = _prog_maps("rung4")
    a, b = engine.env_state_layout(p3, m3), engine.env_state_layout(p3, m3)
    assert a == b
    c = engine.env_state_layout(p4, m4)
    assert c["format"] != a["format"]
    # the same rung-3 program with other maps: the capacities of a lean program do not depend on them
    assert engine.env_state_layout(p3, m3[:1])["format"] == a["format"]


def test_format_follows_aoe_capacities():
    prog, cms = _prog_maps("rung4")
    full = engine.env_state_layout(prog, cms)
    # the same program with maps that hold fewer area-effect and territory sources (healers, fires, flags)
    few = np.stack([prog.class_map(hp.random_map(20, 22, {"wall": 18, "healer": 1, "fire": 1, "hub": 2, "wire": 10, "flag_red": 1},
                                                 {"red": 4, "blue": 4, "green": 4}, s)) for s in (0, 1)])
    thin = engine.env_state_layout(prog, few)
    assert thin["format"] != full["format"]
    assert thin["record_bytes"] <= full["record_bytes"]   # (the capacities differ; 16-byte padding may hide it in the size)
    assert engine.env_state_layout(prog, cms[::-1])["format"] == full["format"]


def test_refused_program_and_bad_arguments():
    L = engine.load_lib()
    bad = (ctypes.c_int32 * 200)()
    maps = (ctypes.c_uint16 * 4)()
    info = engine.EnvStateInfo()
    assert L.mgx_env_state_layout(bad, 200, maps, 1, ctypes.byref(info)) == -3
    assert L.mgx_env_state_layout(bad, 200, maps, 0, ctypes.byref(info)) == -1
    assert L.mgx_save_envs(None, None, 0, None) == -1
    assert L.mgx_load_envs(None, None, 0, None, None) == -1
    assert L.mgx_copy_envs(None, None, None, 0) == -1
    assert L.mgx_env_state_info(None, ctypes.byref(info)) == -1


def test_header_constants_parse():
    assert K.ES_MAGIC == 0x5345584D and K.ES_VERSION >= 1
    assert K.ES_HEADER_BYTES == 32 and K.ES_HEADER_BYTES % K.ES_ALIGN == 0
    assert engine.ENV_BAD_STATE == 128 and engine.ENV_BAD_STATE not in (
        engine.ENV_TOKEN_OVERFLOW, engine.ENV_INVALID_KEY_RANGE, engine.ENV_DEPTH, engine.ENV_TOO_MANY_OBJECTS,
        engine.ENV_TOKEN_POOL, engine.ENV_PROXY_INVENTORY, engine.ENV_AGENT_LIFECYCLE)


@pytest.mark.parametrize("envs,unique", [([], False), ([0, 70], False), ([-1], False), ([1, 1], True), ([[0, 1]], False),
                                          ([0.5], False)])
def test_env_list_validation(envs, unique):
    with pytest.raises(ValueError):
        engine.env_list(np.asarray(envs), 70, "test", unique=unique)


def test_env_list_accepts():
    assert engine.env_list(None, 5, "t").tolist() == [0, 1, 2, 3, 4]
    assert engine.env_list([4, 0], 5, "t", unique=True).tolist() == [4, 0]
    assert engine.env_list([3, 3], 5, "t").tolist() == [3, 3]   # a source may be listed twice
    assert engine.env_list(np.int64(2), 5, "t").tolist() == [2]


def test_env_state_dict_round_trip(tmp_path):
    info = {"record_bytes": 48, "format": 2 ** 63 + 5, "version": 1, "pool_tokens": 64, "n_segments": 3, "reserved": 0}
    data = np.arange(2 * 48, dtype=np.uint8).reshape(2, 48)
    st = engine.EnvState(data, info, [4, 0], {"episode": np.array([2, 3])})
    np.savez(tmp_path / "s.npz", **st.to_dict())
    back = engine.EnvState.from_dict(np.load(tmp_path / "s.npz"))
    assert back.info == info and back.envs.tolist() == [4, 0] and np.array_equal(back.data, data)
    assert back.extra["episode"].tolist() == [2, 3]
    with pytest.raises(ValueError):
        engine.EnvState(data[:, :16], info, [4, 0])


def test_batched_env_checks_lists_before_the_engine():
    from mettagrid_amd.envs import MettaGridBatchedEnv
    prog = compile_spec(presets.rung1_spec(), *presets.rung1_map().shape)
    env = MettaGridBatchedEnv(prog, 3, map_fn=lambda e, ep: prog.class_map(presets.rung1_map()), buffers="host")
    # no reset: there is no engine (and no GPU) — the lists are refused before it is needed
    with pytest.raises(ValueError):
        env.save_state([3])
    with pytest.raises(ValueError):
        env.save_state([])
