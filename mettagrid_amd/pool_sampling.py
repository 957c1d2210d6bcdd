"""Weighted map-pool sampling and per-map episode statistics, restated in numpy (csrc/mgx_pool_sample.h).

The reference's map cache hands every new episode a uniformly random cached map (python/src/mettagrid/simulator/map_cache.py:
207-215, ``rng.integers(0, len(maps_list))``) and its trainers feed per-task returns back into the task distribution; here the
draw is counter-based, so that it does not depend on which envs restart together: the episode ``k`` (the value of the slot's
episode counter after the auto-reset bump) of env slot ``e`` uses

    u = Generator(PCG64(SeedSequence(sample_seed, spawn_key=(a, k)))).integers(0, 2**32, dtype=uint32),  a = (env_offset + e) mod 2**32

the low half of the stream's first output, and plays the smallest map ``m`` with ``u < edge[m]``.  Everything here is exact:
the device computes the same words (tests/test_pool_sampling_host.py, tests/test_gpu_pool_sampling.py).
"""
from __future__ import annotations

import numpy as np

from . import early_reset as er

TWO32 = 1 << 32
Q_SCALE = float(1 << 20)   # fixed point of the per-map return sums
MS_COLUMNS = ("episodes", "terminated", "length_sum", "q_sum", "key_min", "key_max")
MS_EMPTY = np.array([0, 0, 0, 0, 0xFFFFFFFFFFFFFFFF, 0], np.uint64)   # a cleared row


def quantise(weights) -> np.ndarray:
    """Weights (f64 [M], finite, >= 0, not all zero) -> uint64 [M] upper edges of the maps' intervals of [0, 2**32): the running
    sum C_m taken sequentially in f64, edge[m] = floor(C_m / C_{M-1} * 2**32) and edge[M-1] = 2**32.  A zero weight gives an
    empty interval; so may a positive weight below 2**-32 of the total."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0:
        raise ValueError("weights: a non-empty 1-d array")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights: finite and >= 0")
    c = np.empty(w.size, np.float64)
    s = 0.0
    for m in range(w.size):   # (np.cumsum is sequential too, but this is the definition)
        s = s + float(w[m])
        c[m] = s
    if not s > 0.0 or not np.isfinite(s):
        raise ValueError("weights: the total must be positive and finite")
    edges = np.floor(c / s * 4294967296.0).astype(np.uint64)
    edges[-1] = TWO32
    return edges


def draw_words(seed, a, k) -> np.ndarray:
    """uint32 [n]: the draw's uniform word for the stream keys (a[i], k[i]) (see the module docstring), vectorised."""
    a = np.atleast_1d(np.asarray(a, dtype=np.uint64))
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    a, k = np.broadcast_arrays(a, k)
    n = a.size
    u64 = np.uint64
    with np.errstate(over="ignore"):
        w = er.generate_state8(er.seedseq_pool(np.full(n, int(seed), u64), (a.reshape(-1), k.reshape(-1))))
        v = [w[2 * i] | (w[2 * i + 1] << u64(32)) for i in range(4)]
        ih = (v[2] << u64(1)) | (v[3] >> u64(63)); il = (v[3] << u64(1)) | u64(1)
        sh, sl = er.step(np.zeros(n, u64), np.zeros(n, u64), ih, il)
        sh, sl = er.add128(sh, sl, v[0], v[1])
        sh, sl = er.step(sh, sl, ih, il)
        sh, sl = er.step(sh, sl, ih, il)   # next64: step, then the XSL-RR output
        x = sh ^ sl
        rot = sh >> u64(58)
        out = (x >> rot) | (x << ((u64(64) - rot) & u64(63)))
    return (out & er.M32).astype(np.uint32)


def pick(edges, u) -> np.ndarray:
    """int32: the smallest m with u < edges[m]."""
    return np.searchsorted(np.asarray(edges, dtype=np.uint64), np.asarray(u, dtype=np.uint64), side="right").astype(np.int32)


def draws(weights, seed, env_offset, envs, episodes) -> np.ndarray:
    """The pool map that episode ``episodes[i]`` of env slot ``envs[i]`` plays."""
    a = (np.asarray(envs, dtype=np.int64) + int(env_offset)) & 0xFFFFFFFF
    return pick(quantise(weights), draw_words(seed, a, episodes))


def return_key(r) -> np.ndarray:
    """The total-order key of f64 values: all bits flipped if negative, else the sign bit set."""
    b = np.atleast_1d(np.asarray(r, dtype=np.float64)).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def key_return(key: int) -> float:
    b = np.uint64(key)
    b = (b & np.uint64((1 << 63) - 1)) if b >> np.uint64(63) else ~b
    return float(np.array([b], np.uint64).view(np.float64)[0])


def table_dicts(table: np.ndarray) -> list:
    """uint64 [(M + 1)][6] -> one dict per row: episodes, terminated, length_sum, return_sum (= q_sum / 2**20), return_min,
    return_max (None for a row without episodes)."""
    out = []
    for row in np.asarray(table, dtype=np.uint64):
        n = int(row[0])
        out.append({"episodes": n, "terminated": int(row[1]), "length_sum": int(row[2]),
                    "return_sum": int(row[3].astype(np.int64)) / Q_SCALE,
                    "return_min": key_return(int(row[4])) if n else None, "return_max": key_return(int(row[5])) if n else None})
    return out


class MapStatsHost:
    """The device's per-map table, restated from episode-log records (dicts with ``map_index``, ``steps``, ``flags`` and
    ``return_sum``, as ``BatchedMettaGrid.drain_episode_log`` returns them): row ``map_index``, or row M for -1."""

    def __init__(self, n_maps: int, num_agents: int) -> None:
        self.M, self.A = int(n_maps), int(num_agents)
        self.clear()

    def clear(self) -> None:
        self.table = np.tile(MS_EMPTY, (self.M + 1, 1))

    def add(self, records) -> "MapStatsHost":
        t = self.table
        with np.errstate(over="ignore"):
            for r in records:
                m = int(r["map_index"])
                row = t[self.M if m < 0 else m]
                ret = np.float64(r["return_sum"]) / np.float64(self.A)
                row[0] += np.uint64(1)
                row[1] += np.uint64(int(r["flags"]) & 1)
                row[2] += np.uint64(int(r["steps"]))
                row[3] += np.array([np.rint(ret * Q_SCALE)]).astype(np.int64).view(np.uint64)[0]
                key = return_key(ret)[0]
                row[4] = min(row[4], key)
                row[5] = max(row[5], key)
        return self

    def snapshot(self) -> np.ndarray:
        out = self.table.copy()
        self.clear()
        return out
