"""CPU: the map generator's recipe and the host restatement of its kernel (mettagrid_amd/mapgen.py RandomMapSpec,
generated_class_maps) against numpy's own shuffle and the reference's builder as restated by random_map."""
import numpy as np
import pytest

import mapgen_cases as mc
from mettagrid_amd import presets
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import env_state_layout
from mettagrid_amd.mapgen import RandomMapSpec, generated_class_maps, random_class_maps, random_map, shuffled_rows

RECORD_BYTES_BEFORE = 34272   # mgx_env_state_layout of the parent commit for the program below (csrc/mgx_env_state.h is untouched)


@pytest.mark.parametrize("two_teams", [False, True])
@pytest.mark.parametrize("border", mc.BORDERS)
@pytest.mark.parametrize("area", mc.AREAS)
def test_generated_maps_equal_the_numpy_builder(area, border, two_teams):
    prog, spec = mc.case(area, border, two_teams)
    got = generated_class_maps(spec, prog, mc.SEEDS)
    want = random_class_maps(prog, spec.height, spec.width, spec.objects, spec.agents, mc.SEEDS, border_width=border)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    for k, s in enumerate(mc.SEEDS):
        cells = random_map(spec.height, spec.width, spec.objects, spec.agents, int(s), border_width=border)
        assert np.array_equal(got[k], prog.class_map(cells)), (area, border, int(s))


def test_a_recipe_that_overflows_goes_through_the_halving_rule():
    prog, _ = mc.case(64, 1, True)
    spec = RandomMapSpec(3, 66, {"wall": 100, "extractor": 40, "chest": 9}, {"red": 8, "blue": 8}, border_width=1)
    low = spec.lower(prog)
    assert int((low.inner != 0).sum()) == 25 + 10 + 2 + 16   # 100, 40, 9 halved twice beside the 16 agents (165 -> 90 -> 53 <= 64)
    got = generated_class_maps(spec, prog, mc.SEEDS)
    for k, s in enumerate(mc.SEEDS):
        assert np.array_equal(got[k], prog.class_map(spec.random_map(int(s))))
    with pytest.raises(ValueError):   # nothing left to halve
        RandomMapSpec(3, 66, {"wall": 1}, {"red": 40, "blue": 40}, border_width=1).lower(prog)
    with pytest.raises(ValueError):   # the recipe is for another map size than the program's
        RandomMapSpec(5, 66, {"wall": 1}, {"red": 1}, border_width=1).lower(prog)


def test_the_stream_equals_the_committed_numpy_shuffles():
    pairs = mc.fixture()
    assert len(pairs) == 12
    for area, seed, perm in pairs:
        assert np.array_equal(shuffled_rows(np.arange(area, dtype=np.uint16), [seed])[0], perm), (area, seed)
    for area, seed, perm in pairs:   # ... and so do whole maps
        prog, spec = mc.case(area, 1, True)
        assert np.array_equal(generated_class_maps(spec, prog, [seed])[0], mc.maps_from_perm(spec.lower(prog), perm))


def test_the_env_state_record_is_unchanged():
    """The recipe and the base seeds are slot-owned: the record of a rung-3 program is what it was before the generator."""
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(2))
    info = env_state_layout(prog, cms)
    assert info["record_bytes"] == RECORD_BYTES_BEFORE and info["version"] == 1
