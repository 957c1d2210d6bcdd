"""Host: csrc/mgx_mapgen_plan.h (the host-only half of the mgx_set_map_*generator calls) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpu_emu/mapgen_plan_check.cpp, which documents the record format): the
lowered recipes of the three case modules are all accepted; the representative map holds the cells of a generated map; the LDS
bytes and the blob layout are what csrc/mgx_mapgen.h and the engine expect; every refusal keeps its code and text."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

import mapgen_cases as mc
import mapgen_scene_cases as sc
import maze_cases as zc
from mettagrid_amd import presets
from mettagrid_amd.fmt import K
from mettagrid_amd.mapgen import LoweredMaze, LoweredScene, MazeGenSpec, generated_class_maps, maze_geometry, maze_walls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
BAD_ARG, PROGRAM = -1, -3   # include/mgx.h MGX_ERR_BAD_ARG, MGX_ERR_PROGRAM
KIND = {"random": 1, "scene": 2, "maze": 3}


def _array(a) -> list:
    a = np.asarray(a).reshape(-1)
    return [a.size] + [int(v) for v in a]


def record(prog, low) -> str:
    """One record of the program's input for what ``lower(prog)`` returned."""
    head = [int(prog.words[K.H_HEIGHT]), int(prog.words[K.H_WIDTH]), int(prog.words[K.H_NUM_CLASSES])]
    tail = [len(low.rename_off) - 1] + _array(low.rename) + _array(low.rename_off)
    if not isinstance(low, LoweredScene):
        body = [KIND["random"]] + head + [low.border_width, low.border_code, low.inner.size] + _array(low.inner)
    else:
        rooms = [low.room_height, low.room_width, low.n_inst, low.rows, low.cols, low.border_width, low.instance_border_width,
                 low.border_code, low.instance_border_code]
        if isinstance(low, LoweredMaze):
            body = [KIND["maze"]] + head + rooms + [low.algorithm, low.room_size, low.wall_size, low.wall_code, int(low.first_on_root),
                                                     low.key_offset, low.n_sym] + _array(low.symbols)
        else:
            body = [KIND["scene"]] + head + rooms + [int(low.first_on_root), low.n_sym] + _array(low.symbols)
    return " ".join(str(int(v)) for v in body + tail)


def lds_bytes(low) -> int:
    """csrc/mgx_mapgen.h: the random recipe's inner array, MGX_MAPSCENE_LDS_BYTES, MGX_MAZE_LDS_BYTES; u16 each, rounded up to 16 B."""
    if not isinstance(low, LoweredScene):
        words = low.inner.size
    else:
        words = low.height * low.width + low.room_height * low.room_width + low.n_sym
        if isinstance(low, LoweredMaze):
            _, _, cols, rows = maze_geometry(low.room_height, low.room_width, low.room_size, low.wall_size)
            words += max(len(maze_walls(cols, rows)), cols * rows) + cols * rows
    return (words * 2 + 15) & ~15


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(records, lds=None) -> per record ("refused", code, text) or ("ok", kind, lds, off_rename, off_off, what, blob, one)."""
    tmp = tmp_path_factory.mktemp("mapgen_plan")
    exe = str(tmp / "mapgen_plan_check")
    emu = os.path.join(ROOT, "tests", "cpu_emu")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DMGX_CPU_EMU", "-I", emu, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "mettagrid_amd", "csrc"), os.path.join(emu, "mapgen_plan_check.cpp"),
                    "-pthread", "-o", exe], check=True, timeout=300)

    def run(records, lds=None):
        path = str(tmp / "recipes.txt")
        with open(path, "w") as f:
            f.write("\n".join(records) + "\n")
        r = subprocess.run([exe, path] + ([] if lds is None else [lds]), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        lines, out = r.stdout.split("\n"), []
        while lines and lines[0]:
            w = lines.pop(0).split(" ")
            if w[0] == "refused":
                out.append(("refused", int(w[1]), " ".join(w[2:])))
                continue
            assert w[0] == "ok" and w[1::2] == ["kind", "lds", "off_rename", "off_off"]
            what, blob, one = (lines.pop(0).split(" ", 1) for _ in range(3))
            assert (what[0], blob[0], one[0]) == ("what", "blob", "one")
            out.append(("ok", int(w[2]), int(w[4]), int(w[6]), int(w[8]), what[1], bytes.fromhex(blob[1] if len(blob) > 1 else ""),
                        np.array(one[1].split(" "), np.int64)))
        assert len(out) == len(records)
        return out
    return run


def all_cases() -> list:
    """(kind, prog, spec, the module's SEEDS) of the 123 recipes of the three case modules."""
    cases = [("random",) + mc.case(a, b, t) + (mc.SEEDS,) for a in mc.AREAS for b in mc.BORDERS for t in (False, True)]
    cases += [("scene",) + sc.case(c["name"]) + (sc.SEEDS,) for c in sc.CASES]
    cases += [("maze",) + zc.case(c["name"]) + (zc.SEEDS,) for c in zc.CASES]
    return cases


def test_every_case_is_accepted_with_its_cells_lds_and_blob(plan):
    cases = all_cases()
    assert len(cases) == 123
    lows = [spec.lower(prog) for _, prog, spec, _ in cases]
    for (kind, prog, spec, seeds), low, res in zip(cases, lows, plan([record(prog, low) for (_, prog, _, _), low in zip(cases, lows)])):
        assert res[0] == "ok", res
        _, got_kind, lds, off_rename, off_off, _, blob, one = res
        assert got_kind == KIND[kind]
        # the invariant the engine's capacity checks rest on: ONE map holds the cells of every generated map
        maps = generated_class_maps(spec, prog, seeds[:3])
        assert one.size == maps[0].size
        for m in maps:
            assert np.array_equal(np.sort(one), np.sort(m.reshape(-1).astype(np.int64)))
        assert lds == lds_bytes(low)
        # cells | rename | rename_off at 16-byte aligned offsets
        cells = np.ascontiguousarray(low.symbols if isinstance(low, LoweredScene) else low.inner, np.uint16).tobytes()
        rename, off = np.ascontiguousarray(low.rename, np.uint16).tobytes(), np.ascontiguousarray(low.rename_off, np.int32).tobytes()
        assert off_rename == (len(cells) + 15) & ~15 and off_off == (off_rename + len(rename) + 15) & ~15
        assert len(blob) == off_off + len(off)
        assert blob[:len(cells)] == cells and blob[off_rename:off_rename + len(rename)] == rename and blob[off_off:] == off
        assert not any(blob[len(cells):off_rename]) and not any(blob[off_rename + len(rename):off_off])


def _maze4():
    """The 4-instance maze recipe of tests/test_gpu_mapgen_maze.py: 9 x 9 rooms, 49 empty cells, 8 symbols, a 21 x 21 map."""
    spec = MazeGenSpec(9, 9, {"wall": 3, "chest": 1}, {"red": 2, "blue": 2}, num_agents=16, border_width=1, instance_border_width=1)
    prog = zc.program(spec, list(presets.rung3_spec().agents))
    low = spec.lower(prog)
    assert low.n_empty == 49 and low.n_sym == 8
    return prog, low


def _with(low, **changes):
    new = copy.copy(low)
    for k, v in changes.items():
        setattr(new, k, v)
    return new


def test_refusals_keep_their_codes_and_texts(plan):
    prog, maze = _maze4()
    nc = int(prog.words[K.H_NUM_CLASSES])
    sprog, sspec = sc.case("n4_root")
    scene = sspec.lower(sprog)
    rprog, rspec = mc.case(64, 1, True)
    rand = rspec.lower(rprog)
    symbols = maze.symbols.copy()
    symbols[3, 0] = 4000
    inner = rand.inner.copy()
    inner[-1] = mc.TEAM0 + 2
    cases = [
        (prog, _with(maze, border_code=4000), BAD_ARG, f"mgx_set_map_maze_generator: class map holds id 4000 but the program has {nc} classes"),
        (prog, _with(maze, symbols=symbols), BAD_ARG, f"mgx_set_map_maze_generator: class map holds id 4000 but the program has {nc} classes"),
        (prog, _with(maze, rename=np.array([4001] + list(maze.rename[1:]))), BAD_ARG,
         f"mgx_set_map_maze_generator: class map holds id 4001 but the program has {nc} classes"),
        (prog, _with(maze, wall_code=4001), BAD_ARG, f"mgx_set_map_maze_generator: class map holds id 4001 but the program has {nc} classes"),
        (prog, _with(maze, border_width=2), BAD_ARG,
         "mgx_set_map_maze_generator: 4 instances are a grid of 2 x 2 rooms, and rooms, instance borders and the outer border must add up "
         "to the program's 21 x 21 map (they give 23 x 23)"),
        (prog, _with(maze, algorithm=2), BAD_ARG, "mgx_set_map_maze_generator: algorithm 2 is neither kruskal (0) nor dfs (1)"),
        (prog, _with(maze, symbols=np.full((4, 50), maze.wall_code, np.uint16)), BAD_ARG,
         "mgx_set_map_maze_generator: 50 symbols do not fit the 49 empty cells of a room's maze"),
        (prog, _with(maze, rename_off=np.array([0, 9, 8], np.int32)), BAD_ARG, "mgx_set_map_maze_generator: rename offsets must ascend"),
        (prog, _with(maze, wall_code=0), BAD_ARG, "mgx_set_map_maze_generator: the wall code is 0 (empty)"),
        (prog, _with(maze, key_offset=2), BAD_ARG,
         "mgx_set_map_maze_generator: null / negative argument, a key offset other than 0 or 1, or base seeds not given"),
        (sprog, _with(scene, room_height=0), BAD_ARG, "mgx_set_map_scene_generator: null / negative argument, or base seeds not given"),
        (sprog, _with(scene, symbols=np.full((4, 26), 1, np.uint16)), BAD_ARG,
         "mgx_set_map_scene_generator: 26 symbols do not fit the 25 cells of a room"),
        (sprog, _with(scene, rename_off=np.array([0, 1] + list(scene.rename_off[2:]), np.int32)), BAD_ARG,
         "mgx_set_map_scene_generator: more cells of team 0 than entries in its rename table"),
        (sprog, _with(scene, rename_off=scene.rename_off[:2], rename=scene.rename[:scene.rename_off[1]]), BAD_ARG,
         "mgx_set_map_scene_generator: a symbol names team 1 of 1"),
        (rprog, _with(rand, inner=inner), BAD_ARG, "mgx_set_map_generator: an inner cell names team 2 of 2"),
        (rprog, _with(rand, inner=np.full(64, mc.TEAM0, np.uint16)), BAD_ARG,
         "mgx_set_map_generator: more cells of team 0 than entries in its rename table"),
        (rprog, _with(rand, inner=rand.inner[:-1]), BAD_ARG,
         "mgx_set_map_generator: the inner array must hold (H - 2 * border_width) * (W - 2 * border_width) = 64 cells of the program's "
         "3 x 66 map, and base seeds must be given"),
    ]
    assert scene.n_teams == 4 and scene.rename_off[1] == 2 and rand.n_teams == 2
    got = plan([record(p, low) for p, low, _, _ in cases])
    for (_, _, code, text), res in zip(cases, got):
        assert res == ("refused", code, text)


def test_the_lds_variable_lowers_the_limit_and_nothing_else(plan):
    prog, maze = _maze4()
    need = lds_bytes(maze)
    assert need == 2 * (441 + 40 + 25 + 81 + 8) + 10   # 1 190 B, rounded up to a multiple of 16
    rec = [record(prog, maze)]
    for bad in ("12x", "", "-5", " 7", "0x10"):
        assert plan(rec, bad) == [("refused", BAD_ARG, f"mgx_set_map_maze_generator: MGX_MAPGEN_LDS_BYTES = '{bad}' is not a decimal byte count")]
    assert plan(rec, str(need - 16)) == [
        ("refused", PROGRAM, f"mgx_set_map_maze_generator: the map of 441 cells with a room of 81, 25 maze cells, 40 walls and 8 symbols needs "
                             f"{need} B of LDS, the generator's workgroup has {need - 16}")]
    for enough in (str(need), str(10 ** 9)):   # exactly the need; a value above the workgroup's 160 KiB changes nothing
        assert plan(rec, enough)[0][:3] == ("ok", KIND["maze"], need)
    rprog, rspec = mc.case(900, 0, False)
    assert plan([record(rprog, rspec.lower(rprog))], "1799") == [
        ("refused", PROGRAM, "mgx_set_map_generator: the inner area of 900 cells needs 1808 B of LDS, the generator's workgroup has 1799")]
