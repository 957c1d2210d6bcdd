"""Writes tests/golden/mapgen/random_maps.npz: ``np.random.default_rng(seed).shuffle(arange(area))`` for a dozen (area, seed) pairs,
as the numpy that ran this script computed them (2.2.6 when the fixture was made).  The fixture pins the stream: the map
generator restates numpy's SeedSequence / PCG64 / Generator.shuffle and must keep producing these whatever numpy does later."""
import os

import numpy as np

PAIRS = [(1, 0), (2, 1), (3, 5), (63, 12345), (64, 2 ** 31), (65, 2 ** 32 - 1), (127, 7), (128, 0), (129, 2 ** 31), (900, 1),
         (900, 2 ** 32 - 1), (900, 3141592653)]

if __name__ == "__main__":
    out = {"areas": np.array([a for a, _ in PAIRS], np.int64), "seeds": np.array([s for _, s in PAIRS], np.uint64)}
    for k, (area, seed) in enumerate(PAIRS):
        perm = np.arange(area, dtype=np.uint16)
        np.random.default_rng(seed).shuffle(perm)
        out[f"perm_{k}"] = perm
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "random_maps.npz"), **out)
