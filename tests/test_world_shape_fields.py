"""CPU: the lean world kernel's preset shape (MgxWorldShapeR3, csrc/mgx_presets_gen.h) is what the library's own planner
decides for the rung-3 preset — the header is generated from `mgx_world_shape_fields`, a host-only query — and the field
list is the same in C++ (MGX_WORLD_SHAPE_FIELDS, csrc/mgx_world.h) and in Python (gen_presets.WORLD_FIELDS)."""
import os
import re

import pytest

from mettagrid_amd import engine, gen_presets, jit, presets
from mettagrid_amd.compiler import compile_spec

CSRC = os.path.join(os.path.dirname(os.path.abspath(gen_presets.__file__)), "csrc")


def _fields(prog):
    return gen_presets.world_fields_of(prog, engine.load_lib())


def test_field_list_is_the_same_on_both_sides():
    text = open(os.path.join(CSRC, "mgx_world.h")).read()
    m = re.search(r"#define MGX_WORLD_SHAPE_FIELDS\(F\)((?:.*\\\n)*.*)\n", text)
    assert m, "MGX_WORLD_SHAPE_FIELDS not found"
    assert tuple(re.findall(r"F\((\w+)\)", m.group(1))) == gen_presets.WORLD_FIELDS


def test_header_holds_the_planners_decisions_for_the_preset(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MGX_")]:
        monkeypatch.delenv(k)
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    got = _fields(prog)
    assert got == gen_presets.world_fields_in_header()
    by_name = dict(zip(gen_presets.WORLD_FIELDS, got))
    assert (by_name["H"], by_name["W"], by_name["A"], by_name["S"]) == (32, 32, 16, 192)
    assert by_name["gen_prog"] == 3 and by_name["move_fast"] != 0 and by_name["duo"] == 1 and by_name["coop_passes"] == 1


@pytest.mark.parametrize("switch,field", [("MGX_NO_GEN", "gen_prog"), ("MGX_NO_MOVE_FAST", "move_fast"), ("MGX_NO_DUO", "duo"),
                                          ("MGX_WORLD_PASSES_PER_ENV", "coop_passes")])
def test_a_create_time_switch_changes_its_field(switch, field, monkeypatch):
    """... so an engine created under it does not match the preset's shape and keeps the generic kernel."""
    for k in [k for k in os.environ if k.startswith("MGX_")]:
        monkeypatch.delenv(k)
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    monkeypatch.setenv(switch, "1")
    got = dict(zip(gen_presets.WORLD_FIELDS, _fields(prog)))
    assert got[field] == 0 and got != dict(zip(gen_presets.WORLD_FIELDS, gen_presets.world_fields_in_header()))


def test_other_programs_have_other_shapes():
    ref = gen_presets.world_fields_in_header()
    for h, w, slots in ((31, 32, 192), (32, 32, 191)):
        assert _fields(compile_spec(presets.rung3_spec(), h, w, max_objects=slots)) != ref


def test_run_time_specialiser_passes_the_shape_with_its_own_handler_id(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MGX_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("MGX_JIT_CACHE", os.path.join(os.path.dirname(CSRC), ".jit_cache"))
    prog = compile_spec(presets.rung3_spec(), 31, 32, max_objects=192)
    world = jit.plan(prog)["world"]
    define = [a for a in world[1] if a.startswith("-DMGX_JIT_WORLD_SHAPE=")]
    assert len(define) == 1
    vals = [int(x) for x in define[0].split("=", 1)[1].split(",")]
    want = _fields(prog)
    want[gen_presets.WORLD_FIELDS.index("gen_prog")] = jit.JIT_GEN_ID
    assert vals == want
