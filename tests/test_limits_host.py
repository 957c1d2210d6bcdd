"""Host-side limits: what the compiler refuses agrees with mgx_create's structural limits, and the Python names of the
mgx_create_paths bits follow include/mgx.h.  No GPU."""
import os
import re

import pytest

import helpers as hp
from mettagrid_amd import presets
from mettagrid_amd.compiler import UnsupportedFeature, compile_spec
from mettagrid_amd.engine import PATH_BITS
from mettagrid_amd.fmt import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_path_bits_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    bits = {int(b): n.lower() for n, b in re.findall(r"MGX_PATH_(\w+) = 1 << (\d+)", hdr)}
    assert [bits[i] for i in range(len(bits))] == [b.lower() for b in PATH_BITS]
    assert int(re.search(r"MGX_PATH_COUNT = (\d+)", hdr).group(1)) == len(PATH_BITS)


def test_compiler_refuses_what_mgx_create_refuses():
    # agent ids are u8 with 0xFF = none: mgx_create takes at most 254 (its LDS staging allows fewer, test_gpu_limits.py)
    assert K.MAX_AGENTS == 254
    compile_spec(hp.teams_spec(presets.rung3_spec(), 254, 2), 40, 40)
    with pytest.raises(ValueError, match="1..254 agents"):
        compile_spec(hp.teams_spec(presets.rung3_spec(), 255, 2), 40, 40)
    # the handler VM packs slot ids as (id + 2) & 0xFFFF: slot 65534 would read back as -2
    assert K.MAX_OBJECT_SLOTS == 65534
    compile_spec(presets.rung3_spec(), 255, 255, max_objects=65534)
    with pytest.raises(UnsupportedFeature, match="65534 object slots"):
        compile_spec(presets.rung3_spec(), 255, 255, max_objects=65535)
    with pytest.raises(UnsupportedFeature, match="255x255"):
        compile_spec(presets.rung3_spec(), 256, 255, max_objects=64)


def test_limit_scenarios_compile():
    for name in hp.LIMIT_SCENARIOS:
        spec_f, map_f, _, _ = hp.LIMIT_SCENARIOS[name]
        grid = map_f(0)
        prog = hp.compile_scenario(name, spec_f(), *grid.shape)
        prog.class_map(grid)


def _create(prog, grid):
    import ctypes
    import numpy as np
    from mettagrid_amd import engine
    lib = engine.load_lib()
    words = np.ascontiguousarray(prog.words, dtype=np.int32)
    cm = np.ascontiguousarray(prog.class_map(grid)[None], dtype=np.uint16)
    seeds = np.zeros(1, np.uint32)
    h = ctypes.c_void_p()
    rc = lib.mgx_create(words.ctypes.data_as(ctypes.c_void_p), len(words), cm.ctypes.data_as(ctypes.c_void_p),
                        seeds.ctypes.data_as(ctypes.c_void_p), 1, 0, ctypes.byref(h))
    return rc, lib.mgx_last_error().decode()


@pytest.mark.parametrize("limit,at,over,match", [
    ("MAX_HANDLER_NESTING", dict(levels=6), dict(levels=7), "handlers nest deeper than 6 levels"),
    ("VALUE_STACK", dict(levels=3, peak=8), dict(levels=3, peak=9), "more than 8 stack entries"),
    ("MAX_QUERY_DEPTH", dict(levels=3, qdepth=3), dict(levels=3, qdepth=4), "queries nest deeper than 3 levels")])
def test_nesting_past_the_limit_is_refused_at_both_layers(limit, at, over, match, monkeypatch):
    """The compiler takes each limit and refuses one level more; a program built past the limit anyway (the compiler's
    limit lifted) is refused by mgx_create before it touches the GPU."""
    grid = hp.nesting_map(0)
    compile_spec(hp.nesting_spec(**at), *grid.shape)
    with pytest.raises(UnsupportedFeature):
        compile_spec(hp.nesting_spec(**over), *grid.shape)
    monkeypatch.setattr(K, limit, getattr(K, limit) + 1)
    prog = compile_spec(hp.nesting_spec(**over), *grid.shape)
    rc, msg = _create(prog, grid)
    assert rc == -3 and match in msg, (rc, msg)


def test_on_use_frames_count_the_move_handler():
    """An on_use tree runs above the move handler that reached it: six levels compile, but need seven VM frames."""
    grid = hp.nesting_map(0)
    rc, msg = _create(compile_spec(hp.nesting_spec(6), *grid.shape), grid)
    assert rc == -3 and "handlers nest deeper than 6 levels" in msg, (rc, msg)
