"""Host only: the weighted map-pool draw, its thresholds and the per-map table (include/mgx.h "Weighted map-pool sampling";
csrc/mgx_pool_sample.h), through the numpy restatement (mettagrid_amd/pool_sampling.py) and the engine-less entry points
mgx_pool_quantise / mgx_pool_draw_words, which run the device kernel's source on the host.  Every comparison is exact."""
import numpy as np
import pytest

from mettagrid_amd import engine
from mettagrid_amd import pool_sampling as ps

U32 = 2**32 - 1


def numpy_word(seed: int, a: int, k: int) -> int:
    """The definition: numpy's own generator."""
    g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed), spawn_key=(int(a), int(k)))))
    return int(g.integers(0, 2**32, dtype=np.uint32))


def lib_words(seed, a, k) -> np.ndarray:
    a, k = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.uint32)
    out = np.zeros(a.size, np.uint32)
    assert engine.load_lib().mgx_pool_draw_words(int(seed), a.ctypes.data, k.ctypes.data, int(a.size), out.ctypes.data) == 0
    return out


def lib_quantise(w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.full(max(w.size, 1), 77, np.uint64)
    rc = engine.load_lib().mgx_pool_quantise(w.ctypes.data, int(w.size), out.ctypes.data)
    return rc, out[:w.size]


def test_known_answer():
    assert numpy_word(12345, 7, 3) == 652139049   # (numpy 2.2.6; the stream is frozen by numpy's compatibility policy)
    assert int(ps.draw_words(12345, [7], [3])[0]) == 652139049
    assert int(lib_words(12345, [7], [3])[0]) == 652139049


def test_draw_words_equal_numpys_generator():
    rng = np.random.default_rng(2024)
    triples = [tuple(int(x) for x in t) for t in rng.integers(0, 2**32, (500, 3))]
    corners = [0, U32]
    triples += [(s, a, k) for s in corners for a in corners for k in corners]
    triples += [(12345, 7, 3), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    want = np.array([numpy_word(*t) for t in triples], np.uint32)
    by_seed: dict = {}
    for i, (s, a, k) in enumerate(triples):
        by_seed.setdefault(s, []).append(i)
    got_py, got_lib = np.zeros_like(want), np.zeros_like(want)
    for s, idx in by_seed.items():   # (both forms take one seed and arrays of keys)
        a = [triples[i][1] for i in idx]
        k = [triples[i][2] for i in idx]
        got_py[idx] = ps.draw_words(s, a, k)
        got_lib[idx] = lib_words(s, a, k)
    assert np.array_equal(got_py, want)
    assert np.array_equal(got_lib, want)


def test_one_word_keys_still_match_numpy():
    """seedseq_pool's tuple key did not move the one-word form the map generators use."""
    from mettagrid_amd import early_reset as er
    seeds = np.array([0, 1, 99, U32], np.uint64)
    with np.errstate(over="ignore"):
        for key in (0, 3, U32):
            got = np.stack(er.generate_state8(er.seedseq_pool(seeds, key)), axis=1).astype(np.uint32)
            same = np.stack(er.generate_state8(er.seedseq_pool(seeds, (key,))), axis=1).astype(np.uint32)
            want = np.stack([np.random.SeedSequence(int(s), spawn_key=(key,)).generate_state(8) for s in seeds])
            assert np.array_equal(got, want) and np.array_equal(same, want)


def test_thresholds():
    assert ps.quantise([1, 1, 2]).tolist() == [2**30, 2**31, 2**32]
    assert ps.quantise(np.ones(8)).tolist() == [(m + 1) * 2**29 for m in range(8)]
    assert ps.quantise([5.0]).tolist() == [2**32]
    e = ps.quantise([3, 0, 1, 0.5, 0])
    assert e[1] == e[0] and e[4] == 2**32 and e[3] == 2**32     # zero weights: empty intervals (the last edge is always 2**32)
    tiny = ps.quantise([0.25, 2.0**-40, 1.0])
    assert tiny[1] == tiny[0]                                    # a positive weight below 2**-32 of the total may get none
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 16, 17, 1000):
        for w in (rng.random(n), rng.random(n) * (rng.random(n) < 0.5) + (np.arange(n) == n // 2), rng.exponential(1e6, n), rng.random(n) * 1e-300):
            want = ps.quantise(w)
            rc, got = lib_quantise(w)
            assert rc == 0 and np.array_equal(got, want), (n, w)
            assert want.dtype == np.uint64 and (np.diff(want.astype(np.int64)) >= 0).all() and want[-1] == 2**32
            assert (want[:-1] <= 2**32).all()


@pytest.mark.parametrize("bad", [[], [1.0, -1.0], [1.0, -0.5, 2.0], [float("nan"), 1.0], [1.0, float("inf")], [-float("inf"), 1.0],
                                 [0.0, 0.0], [0.0], [1e308, 1e308]])
def test_refusals(bad):
    with pytest.raises(ValueError):
        ps.quantise(bad)
    rc, out = lib_quantise(bad)
    assert rc == -1 and (out == 77).all()   # MGX_ERR_BAD_ARG, nothing written
    assert b"mgx_pool_quantise" in engine.load_lib().mgx_last_error()


def test_picks():
    rng = np.random.default_rng(3)
    for w in ([1, 1, 2], [3, 0, 1, 0.5], [0, 0, 1], [1], rng.random(37)):
        edges = ps.quantise(w)
        u = np.concatenate([rng.integers(0, 2**32, 2000, dtype=np.uint64), [0, U32], edges[:-1], np.maximum(edges, 1) - 1]).astype(np.uint64)
        u = u[u <= U32]
        got = ps.pick(edges, u)
        assert np.array_equal(got, np.searchsorted(edges, u, side="right"))
        slow = np.array([min(m for m in range(len(edges)) if x < edges[m]) for x in u[:300]])
        assert np.array_equal(got[:300], slow)
        assert (np.asarray(w, dtype=np.float64)[got] > 0).all()


FREQ_SEED = 0   # chosen on the CPU: numpy's own generator meets the bounds below at this seed, so the outcome is fixed


def test_frequencies():
    """The 65 536 draws of a < 256, k < 256 at one seed, weights [3, 0, 1, 0.5]: not statistical, numpy alone decides."""
    w = np.array([3, 0, 1, 0.5])
    a, k = (x.reshape(-1) for x in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    u = np.array([numpy_word(FREQ_SEED, x, y) for x, y in zip(a, k)], np.uint32)
    assert np.array_equal(ps.draw_words(FREQ_SEED, a, k), u)
    assert np.array_equal(lib_words(FREQ_SEED, a, k), u)
    counts = np.bincount(ps.pick(ps.quantise(w), u), minlength=4)
    assert counts[1] == 0 and counts.sum() == 65536
    n, p = 65536, w / w.sum()
    for m in (0, 2, 3):
        assert abs(counts[m] - n * p[m]) <= 5 * np.sqrt(n * p[m] * (1 - p[m])), (m, counts)


def test_map_stats_restatement():
    A = 4
    h = ps.MapStatsHost(3, A)
    assert np.array_equal(h.table, np.tile(ps.MS_EMPTY, (4, 1)))
    recs = [{"map_index": 0, "steps": 5, "flags": 1, "return_sum": 2.0},      # r = 0.5
            {"map_index": 0, "steps": 7, "flags": 2, "return_sum": -6.0},     # r = -1.5
            {"map_index": 2, "steps": 3, "flags": 5, "return_sum": 4 * (2.0**-21)},   # r = 2**-21: q = rint(0.5) = 0 (half to even)
            {"map_index": 2, "steps": 3, "flags": 0, "return_sum": 4 * 3 * (2.0**-21)},  # q = rint(1.5) = 2
            {"map_index": -1, "steps": 11, "flags": 6, "return_sum": -4 * (2.0**-20)}]   # unattributed, q = -1
    t = h.add(recs).table
    key = lambda r: int(ps.return_key(r)[0])
    assert t[0].tolist() == [2, 1, 12, (-(1 << 20)) % 2**64, key(-1.5), key(0.5)]
    assert t[1].tolist() == ps.MS_EMPTY.tolist()
    assert t[2].tolist() == [2, 1, 6, 2, key(2.0**-21), key(3 * 2.0**-21)]
    assert t[3].tolist() == [1, 0, 11, 2**64 - 1, key(-(2.0**-20)), key(-(2.0**-20))]
    # the key is the total order of f64
    vals = np.array([-np.inf, -2.5, -1e-300, -0.0, 0.0, 1e-300, 1.0, np.inf])
    keys = ps.return_key(vals)
    assert (np.diff(keys.astype(object)) > 0).all()
    assert [ps.key_return(int(x)) for x in keys] == vals.tolist() and np.signbit(ps.key_return(int(keys[3])))
    d = ps.table_dicts(h.snapshot())
    assert d[0] == {"episodes": 2, "terminated": 1, "length_sum": 12, "return_sum": -1.0, "return_min": -1.5, "return_max": 0.5}
    assert d[1] == {"episodes": 0, "terminated": 0, "length_sum": 0, "return_sum": 0.0, "return_min": None, "return_max": None}
    assert d[3]["return_sum"] == -(2.0**-20) and d[3]["return_min"] == d[3]["return_max"] == -(2.0**-20)
    assert np.array_equal(h.table, np.tile(ps.MS_EMPTY, (4, 1)))   # the snapshot cleared it


def test_header_columns():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")).read()
    names = re.search(r"enum \{ (MGX_MS_EPISODES.*?)\};", hdr, flags=re.S).group(1).replace("\n", " ").split(",")
    got = [n.split("=")[0].strip()[len("MGX_MS_"):].lower() for n in names]
    assert got == list(ps.MS_COLUMNS) + ["count"]
