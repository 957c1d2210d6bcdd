"""build()-time specialisation: the shapes of the benchmark presets as compile-time constants for the observation kernel
and the lean world kernel.

``python -m mettagrid_amd.gen_presets`` compiles the preset programs (BASELINE.json configs[2] and configs[3], at the
shapes bench.py runs them) and writes ``csrc/mgx_presets_gen.h`` with one ``MgxObsShape<...>`` per preset.  The engine
launches that instance of ``mgx_obs_kernel`` when a program's shape equals it (``mgx_obs_shape_matches``, checked field by
field at ``mgx_create``) and the generic, run-time-shaped kernel for every other program — a preset whose definition
changes without a rebuild simply stops matching.

The lean world kernel's shape (``MgxWorldShapeR3``, ``MgxWorldShape`` in csrc/mgx_world.h) holds the planner's decisions
beside the sizes, so its values come from the planner itself: ``sync_world(lib)`` asks the library just built
(``mgx_world_shape_fields``: host-only) and rewrites the header when they differ, and build() then compiles once more.  The
committed header holds the values of the committed preset, so a clean checkout builds once.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

from . import presets
from .compiler import compile_spec
from .fmt import K

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "csrc", "mgx_presets_gen.h")


def shape_of(prog) -> dict:
    """The fields of MgxObsShape (csrc/mgx_obs.h) for a compiled program, as mgx_create derives them from the blob."""
    w = prog.words
    sec = lambda s: int(w[K.H_SECTION_BASE + 2 * s])        # noqa: E731
    cnt = lambda s: int(w[K.H_SECTION_BASE + 2 * s + 1])    # noqa: E731
    nc = int(w[K.H_NUM_CLASSES])
    cls = [w[sec(K.SEC_CLASSES) + c * K.C_WORDS: sec(K.SEC_CLASSES) + (c + 1) * K.C_WORDS] for c in range(nc)]
    nrw = max([1] + [int(c[K.C_REWARD_COUNT]) for c in cls])
    any_aoe = any(int(c[K.C_AOE_COUNT]) > 0 for c in cls)
    extended = (any_aoe or int(w[K.H_NUM_TERRITORIES]) > 0 or int(w[K.H_NUM_SCHEDULE]) > 0 or int(w[K.H_NUM_MATQ]) > 0 or
                int(w[K.H_GAME_ON_TICK]) >= 0 or int(w[K.H_DYNAMIC_TAGS]) != 0 or cnt(K.SEC_QUERIES) > 0)
    # rewards evaluated beside the token-list phase: no stat / query operand in any reward expression (lean games only)
    pure = not extended
    for k in range(cnt(K.SEC_REWARDS)):
        rw = w[sec(K.SEC_REWARDS) + k * K.RW_WORDS: sec(K.SEC_REWARDS) + (k + 1) * K.RW_WORDS]
        for i in range(int(rw[K.RW_GV_COUNT])):
            op = int(w[sec(K.SEC_GV_CODE) + (int(rw[K.RW_GV_START]) + i) * K.GV_WORDS + K.GV_OP])
            if op in (K.GOP_STAT, K.GOP_QUERY_INVENTORY, K.GOP_QUERY_COUNT):
                pure = False
    return dict(H=int(w[K.H_HEIGHT]), W=int(w[K.H_WIDTH]), A=int(w[K.H_NUM_AGENTS]), S=int(w[K.H_MAX_OBJECTS]), T=int(w[K.H_NUM_TOKENS]),
                NOFF=int(w[K.H_NUM_OBS_OFFSETS]), BASE=int(w[K.H_TOKEN_BASE]), NOV=int(w[K.H_NUM_OBS_VALUES]),
                NT=int(w[K.H_NUM_TERRITORIES]), NRW=nrw, FLAGS=int(w[K.H_GLOBAL_FLAGS]), MAX_STEPS=int(w[K.H_MAX_STEPS]),
                BLKW=sec(K.SEC_WORDLIST) - sec(K.SEC_INV_FEATURES), MASK_FEAT=int(w[K.H_FEAT_BASE + K.F_AOE_MASK]),
                REWARDS_EARLY=1 if pure else 0, extended=extended)


FIELDS = ("H", "W", "A", "S", "T", "NOFF", "BASE", "NOV", "NT", "NRW", "FLAGS", "MAX_STEPS", "BLKW", "MASK_FEAT", "REWARDS_EARLY")


def preset_shapes() -> dict:
    r3 = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    r4 = compile_spec(presets.rung4_spec(), 64, 64, max_objects=presets.RUNG4_MAX_OBJECTS)
    return {"R3": shape_of(r3), "R4": shape_of(r4)}


# MGX_WORLD_SHAPE_FIELDS of csrc/mgx_world.h, in its order (tests/test_world_shape_fields.py keeps the two equal)
WORLD_FIELDS = ("H", "W", "A", "S", "NSP", "NSW", "NG", "NGW", "SEENW", "nact", "max_priority", "flags", "hp_res", "n_move_handlers",
                "any_on_tick", "tick_in_aoe", "flat_top", "defer_book", "shadow", "gen_prog", "duo", "tick_split", "coop_passes",
                "move_fast", "mf_lds_off", "mf_dirty_words", "mf_exact", "act_ngset", "act_kinds", "act_args_lo", "act_args_hi")


def act_kind(fields, a: int) -> int:
    """Kind of action ``a`` from the packed action table of a world shape (csrc/mgx_world.h mgx_act_kind)."""
    by = dict(zip(WORLD_FIELDS, fields))
    return ((by["act_kinds"] & 0xFFFFFFFF) >> (2 * a)) & 3


def act_arg(fields, a: int) -> int:
    """... and its argument (mgx_act_arg): actions 0-7 in act_args_lo, 8-15 in act_args_hi, four bits each."""
    by = dict(zip(WORLD_FIELDS, fields))
    return ((by["act_args_lo" if a < 8 else "act_args_hi"] & 0xFFFFFFFF) >> (4 * (a & 7))) & 15

_WORLD_RE = re.compile(r"^typedef MgxWorldShape\w*(?:<([-0-9, ]+)>)? MgxWorldShapeR3;", re.M)


def world_fields_in_header():
    """The values of MgxWorldShapeR3 in the header as it stands (None: no header, or the placeholder)."""
    try:
        m = _WORLD_RE.search(open(OUT).read())
    except OSError:
        return None
    return [int(x) for x in m.group(1).split(",")] if m and m.group(1) else None


def world_fields_of(prog, lib) -> list:
    """MGX_WORLD_SHAPE_FIELDS of a compiled program as the planner of ``lib`` (a loaded libmgx) derives them under the
    process's create-time switches: host-only."""
    import ctypes as C

    import numpy as np
    words = np.ascontiguousarray(prog.words, dtype=np.int32)
    lib.mgx_world_shape_fields.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32]
    lib.mgx_world_shape_fields.restype = C.c_int32
    out = np.zeros(64, dtype=np.int32)
    n = lib.mgx_world_shape_fields(words.ctypes.data, words.size, out.ctypes.data, out.size)
    if n != len(WORLD_FIELDS):
        raise RuntimeError(f"mgx_world_shape_fields: {n}")
    return [int(x) for x in out[:n]]


def world_fields_from(lib_path: str) -> list:
    """... of the rung-3 preset (run in a process of its own by sync_world, with every create-time switch at its default)."""
    import ctypes as C
    return world_fields_of(compile_spec(presets.rung3_spec(), 32, 32, max_objects=192), C.CDLL(lib_path))


def sync_world(lib_path: str) -> bool:
    """Make MgxWorldShapeR3 in the header equal to what the planner of the library just built decides for the preset.
    True: the header changed, the units that include it must be compiled again."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGX_")}
    res = subprocess.run([sys.executable, "-m", "mettagrid_amd.gen_presets", "--world-fields", lib_path], capture_output=True, text=True,
                         cwd=os.path.dirname(_HERE), env=env)
    if res.returncode != 0:
        raise RuntimeError(f"gen_presets --world-fields failed: {res.stderr[-2000:]}")
    fields = [int(x) for x in res.stdout.split()]
    if fields == world_fields_in_header():
        return False
    open(OUT, "w").write(render(fields))
    return True


def render(world_fields=None) -> str:
    if world_fields is None:
        world_fields = world_fields_in_header()
    lines = ["// GENERATED by mettagrid_amd/gen_presets.py at build() — the shapes of the benchmark presets (BASELINE.json configs[2], [3])",
             "// for the specialised instances of mgx_obs_kernel.  Field order: " + ", ".join(FIELDS) + ".",
             "#ifndef MGX_PRESETS_GEN_H_", "#define MGX_PRESETS_GEN_H_", "#ifdef MGX_OBS_H_"]
    for name, sh in preset_shapes().items():
        lines.append(f"typedef MgxObsShape<{', '.join(str(sh[f]) for f in FIELDS)}> MgxObsShape{name};   // extended = {int(sh['extended'])}")
        if name == "R3":   # the same game with an episode length set (max_steps read at run time): the env wrappers' configuration
            anylen = dict(sh, MAX_STEPS=-1)
            lines.append(f"typedef MgxObsShape<{', '.join(str(anylen[f]) for f in FIELDS)}> MgxObsShape{name}AnyLength;")
    lines += ["#endif  // MGX_OBS_H_",
              "// ... and of the lean world kernel (configs[2]): the fields of MGX_WORLD_SHAPE_FIELDS (mgx_world.h) in that order, as the",
              "// planner decides them (mgx_world_shape_fields, gen_presets.sync_world)."]
    if world_fields:
        lines.append(f"typedef MgxWorldShape<{', '.join(str(v) for v in world_fields)}> MgxWorldShapeR3;")
    else:   # first build of a tree without the header: matches no program; sync_world fills it in
        lines.append("typedef MgxWorldShapeDyn MgxWorldShapeR3;")
    lines += ["#endif  // MGX_PRESETS_GEN_H_", ""]
    return "\n".join(lines)


def main() -> None:
    text = render()
    if not os.path.exists(OUT) or open(OUT).read() != text:
        open(OUT, "w").write(text)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--world-fields":
        print(" ".join(str(v) for v in world_fields_from(sys.argv[2])))
    else:
        main()
