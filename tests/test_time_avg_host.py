"""Host only: the time averages' C ABI where it needs no GPU — the layout words (mgx_time_average_layout_of: the engine-free form
of mgx_time_average_layout, the same function behind both), argument refusals, and the Python surface's own checks."""
import ctypes

import numpy as np
import pytest

from mettagrid_amd import engine, presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.envs import MettaGridBatchedEnv

TAL = {k: i for i, k in enumerate(BatchedMettaGrid.TAL)}


def _layout(ng: int, cap: int) -> np.ndarray:
    out = np.full(len(TAL) + 1, -77, np.int32)
    assert engine.load_lib().mgx_time_average_layout_of(ng, cap, out.ctypes.data) == 0
    assert out[-1] == -77   # exactly MGX_TAL_COUNT words are written
    return out[:-1]


@pytest.mark.parametrize("ng", [0, 1, 31, 32, 33, 64, 65, 200])
def test_layout_words_are_consistent(ng):
    w = _layout(ng, 5)
    g = lambda k: int(w[TAL[k]])  # noqa: E731
    assert g("NG") == ng and g("SEEN_WORDS") == (ng + 31) // 32 and g("LOG_CAPACITY") == 5
    assert g("HEADER_WORDS") == 8 and g("OFF_AVG") == g("HEADER_WORDS") and g("OFF_AVG") % 2 == 0      # f64 columns on 8-byte boundaries
    assert g("OFF_SEEN") == g("OFF_AVG") + 2 * ng
    assert g("REC_WORDS") >= g("OFF_SEEN") + g("SEEN_WORDS") and g("REC_WORDS") % 4 == 0 and g("REC_WORDS") - (g("OFF_SEEN") + g("SEEN_WORDS")) < 4
    assert g("LOG_WORDS") == g("REC_WORDS")
    assert g("TOTALS_HEADER") == 2 and g("TOTALS_WORDS") == 2 + 2 * ng


def test_header_enums_match_the_python_names():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")).read()
    m = re.search(r"enum \{ (MGX_TAL_NG = 0.*?) \};", hdr, flags=re.S)
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names == ["MGX_TAL_" + k for k in BatchedMettaGrid.TAL] + ["MGX_TAL_COUNT"]


def test_refusals_without_an_engine():
    L = engine.load_lib()
    out = np.zeros(len(TAL), np.int32)
    assert L.mgx_time_average_layout_of(-1, 0, out.ctypes.data) == -1 and b"mgx_time_average_layout_of" in L.mgx_last_error()
    assert L.mgx_time_average_layout_of(3, -1, out.ctypes.data) == -1
    assert L.mgx_time_average_layout_of(3, 0, None) == -1
    assert L.mgx_set_time_averages(None, 1, 0) == -1 and b"mgx_set_time_averages" in L.mgx_last_error()
    assert L.mgx_time_average_layout(None, out.ctypes.data) == -1
    assert L.mgx_request_time_averages(None) == -1
    ready = ctypes.c_int32(5)
    assert L.mgx_fetch_time_averages(None, 0, out.ctypes.data, ctypes.byref(ready)) == -1
    assert L.mgx_drain_time_average_log(None, out.ctypes.data, 1, ctypes.byref(ready), None) == -1
    assert L.mgx_get_time_average_state(None, out.ctypes.data, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert L.mgx_put_time_average_state(None, out.ctypes.data, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1


def test_wrapper_refuses_time_averages_without_episode_stats():
    prog = compile_spec(presets.rung2_spec(), 32, 32)
    with pytest.raises(ValueError, match="episode_stats"):
        MettaGridBatchedEnv(prog, 2, map_fn=lambda e, ep: None, episode_stats=False, time_averaged_stats=True)
    assert MettaGridBatchedEnv(prog, 2, map_fn=lambda e, ep: None).time_averaged_stats is False
