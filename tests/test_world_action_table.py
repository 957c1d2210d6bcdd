"""CPU: the action table as constants of the lean world kernel's shape (csrc/mgx_world.h mgx_act_kind / mgx_act_arg;
MgxDev::act_kinds, act_args_lo, act_args_hi packed by the planner, csrc/mgx_plan.h).  The committed header's three values are
the planner's for the preset, and they decode to the action list compile_spec emits: noop, the move directions with their
orientation, the vibes with their index."""
import os

from mettagrid_amd import engine, gen_presets, presets
from mettagrid_amd.compiler import ORIENTATIONS, compile_spec

PACKED = ("act_kinds", "act_args_lo", "act_args_hi")
NOOP, MOVE, VIBE = 0, 1, 2   # include/mgx_program.h MGX_AK_*


def _expected(spec, prog):
    out = []
    for name in prog.action_names:
        if name == "noop":
            out.append((NOOP, 0))
        elif name.startswith("move_"):
            out.append((MOVE, ORIENTATIONS[name[len("move_"):]]))
        else:
            assert name.startswith("change_vibe_"), name
            out.append((VIBE, list(spec.vibe_names).index(name[len("change_vibe_"):])))
    return out


def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MGX_")]:
        monkeypatch.delenv(k)


def test_header_constants_are_the_planners_and_decode_to_the_action_list(monkeypatch):
    _clean_env(monkeypatch)
    spec = presets.rung3_spec()
    prog = compile_spec(spec, 32, 32, max_objects=192)
    header = gen_presets.world_fields_in_header()
    planned = gen_presets.world_fields_of(prog, engine.load_lib())
    at = [gen_presets.WORLD_FIELDS.index(f) for f in PACKED]
    assert [header[i] for i in at] == [planned[i] for i in at]
    assert header[at[0]] != -1, "the preset's table fits the packed form"
    want = _expected(spec, prog)
    assert len(want) == 13 == planned[gen_presets.WORLD_FIELDS.index("nact")]
    assert [(gen_presets.act_kind(header, a), gen_presets.act_arg(header, a)) for a in range(len(want))] == want


def test_another_action_list_packs_to_other_constants(monkeypatch):
    """One move direction fewer: every later action moves down one place, and the decode follows."""
    import dataclasses
    _clean_env(monkeypatch)
    base = presets.rung3_spec()
    spec = dataclasses.replace(base, move_directions=list(base.move_directions[:7]))
    prog = compile_spec(spec, 32, 32, max_objects=192)
    got = gen_presets.world_fields_of(prog, engine.load_lib())
    ref = gen_presets.world_fields_in_header()
    at = [gen_presets.WORLD_FIELDS.index(f) for f in PACKED]
    assert [got[i] for i in at] != [ref[i] for i in at]
    want = _expected(spec, prog)
    assert [(gen_presets.act_kind(got, a), gen_presets.act_arg(got, a)) for a in range(len(want))] == want
