"""Host only: the record / totals layout of the per-policy episode statistics (include/mgx.h "Per-policy episode statistics")
through the test aid mgx_policy_stats_layout_of, which needs no GPU."""
import numpy as np
import pytest

from mettagrid_amd import engine
from mettagrid_amd.engine import BatchedMettaGrid

MAXP = BatchedMettaGrid.MAX_POLICIES


def _layout(NS, A, P, cap=0):
    L = engine.load_lib()
    out = np.full(len(BatchedMettaGrid.PSL), -1, np.int32)
    rc = L.mgx_policy_stats_layout_of(NS, A, P, cap, out.ctypes.data)
    return rc, {k: int(v) for k, v in zip(BatchedMettaGrid.PSL, out)}


def test_max_policies_is_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")).read()
    assert int(re.search(r"#define\s+MGX_MAX_POLICIES\s+(\d+)", hdr).group(1)) == MAXP
    names = re.search(r"enum \{ (MGX_PSL_NS.*?)\};", hdr, flags=re.S).group(1).replace("\n", " ").split(",")
    assert [n.split("=")[0].strip()[len("MGX_PSL_"):] for n in names][:-1] == list(BatchedMettaGrid.PSL) and names[-1].strip() == "MGX_PSL_COUNT"


@pytest.mark.parametrize("NS", [0, 1, 31, 32, 33, 64, 65, 200])
@pytest.mark.parametrize("P", [1, 2, 3, 8, MAXP])
def test_layout_words(NS, P):
    rc, w = _layout(NS, 6, P, cap=5)
    assert rc == 0
    nsw = (NS + 31) // 32
    assert (w["NS"], w["A"], w["P"], w["SEEN_WORDS"], w["LOG_CAPACITY"]) == (NS, 6, P, nsw, 5)
    # the record: fields in ascending order without overlap, inside the record
    fields = [(w["HEADER_WORDS"], 0), (w["OFF_REWARD"], 2 * P), (w["OFF_COUNT"], P), (w["OFF_SUM"], 2 * P * NS), (w["OFF_BITS"], P * nsw)]
    assert w["HEADER_WORDS"] == 4
    end = w["HEADER_WORDS"]
    for off, size in fields[1:]:
        assert off >= end, (fields, w)
        end = off + size
    assert end <= w["REC_WORDS"] < end + 4
    assert w["OFF_REWARD"] % 2 == 0 and w["OFF_SUM"] % 2 == 0            # f64 fields on 8-byte boundaries
    assert w["REC_WORDS"] % 4 == 0 and w["LOG_WORDS"] == w["REC_WORDS"]   # records on 16-byte boundaries
    # the totals
    assert w["TOTALS_HEADER"] == 1 and w["TOTALS_POLICY_WORDS"] == 5
    assert w["TOTALS_OFF_SUM"] == w["TOTALS_HEADER"] + w["TOTALS_POLICY_WORDS"] * P
    assert w["TOTALS_OFF_COUNT"] == w["TOTALS_OFF_SUM"] + P * NS and w["TOTALS_WORDS"] == w["TOTALS_OFF_COUNT"] + P * NS


def test_policy_count_limits():
    assert _layout(10, 4, 1)[0] == 0 and _layout(10, 4, MAXP)[0] == 0
    for P in (0, -1, MAXP + 1):
        rc, w = _layout(10, 4, P)
        assert rc == -1 and w["REC_WORDS"] == -1     # MGX_ERR_BAD_ARG, nothing written
        assert b"policies" in engine.load_lib().mgx_last_error()
    assert _layout(-1, 4, 2)[0] == -1 and _layout(10, 0, 2)[0] == -1 and _layout(10, 4, 2, cap=-1)[0] == -1
