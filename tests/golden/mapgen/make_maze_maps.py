"""Writes tests/golden/mapgen/maze_cases.json and maze_maps.npz: for every recipe of tests/maze_cases.py the reference's own
``MapGen.Config`` with a ``Maze.Config`` instance and a ``Random.Config`` child (its ``model_dump(mode="json")``) and the grids
``MapGen(config with seed).build()`` gives for a handful of seeds, each as an index array into the case's sorted symbol list.
Data only: the reference is imported from where it lies (MGX_REFERENCE) and nothing of it is copied.  The fixtures pin what
mettagrid_amd.mapgen.MazeGenSpec restates."""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # tests
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

if __name__ == "__main__":
    import make_reference_fixtures as mrf
    mrf._py310_shims()
    sys.path.insert(0, mrf.REF_PY)
    from mettagrid.mapgen.mapgen import MapGen
    from mettagrid.mapgen.scene import ChildrenAction
    from mettagrid.mapgen.scenes.maze import Maze
    from mettagrid.mapgen.scenes.random import Random

    import maze_cases as zc

    cases, arrays = {}, {}
    for c in zc.CASES:
        kw = zc.spec_kwargs(c)
        child = Random.Config(objects=kw.pop("objects"), agents=kw.pop("agents"))
        scene = Maze.Config(algorithm=kw.pop("algorithm"), room_size=kw.pop("room_size"), wall_size=kw.pop("wall_size"),
                            children=[ChildrenAction(scene=child, where="full")])
        cfg = MapGen.Config(instance=scene, **kw)
        grids = {seed: MapGen(cfg.model_copy(update={"seed": seed})).build().grid for seed in zc.FIXTURE_SEEDS}
        symbols = sorted({str(s) for g in grids.values() for s in g.reshape(-1)})
        index = {s: i for i, s in enumerate(symbols)}
        cases[c["name"]] = {"config": cfg.model_dump(mode="json"), "seeds": list(zc.FIXTURE_SEEDS), "symbols": symbols}
        for seed, g in grids.items():
            arrays[f"{c['name']}_{seed}"] = np.array([[index[str(s)] for s in row] for row in g], dtype=np.uint8)
    with open(os.path.join(HERE, "maze_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)   # (key order is data: the objects of a scene are placed in dict order)
        f.write("\n")
    # an .npz is a zip of .npy members; written here with a fixed member time, so that the same arrays give the same bytes
    with zipfile.ZipFile(os.path.join(HERE, "maze_maps.npz"), "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[name], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
