"""GPU: the run-time specialised kernels (mettagrid_amd/jit.py, mgx_attach_code) over the case table of tests/jit_cases.py:
generated handler code, folded world shapes and folded observation shapes that tests/test_gpu_jit.py's three programs do
not have.  Every case runs 45 envs — one full wavefront of 32 (the flat, wavefront-cooperative form of the batched passes)
and one of 13 — beside a `specialize=False` twin, compared on every env after every step, and beside the oracle on envs 0,
31, 32 and 44; at step 10 envs 1 and 32 restart onto other maps and seeds.  Bit equality throughout."""
import pytest

import jit_cases as jc

pytestmark = pytest.mark.gpu
RESTART_AT, RESTART_ENVS = jc.RESTART_AT, jc.RESTART_ENVS


@pytest.fixture(scope="module")
def compiled():
    """Every code object of the table, compiled once and together (the wait of the session is paid here)."""
    jobs = jc.wait_for()
    with jc.cache_env():
        yield jobs


def _run(tw: "jc.Twin") -> None:
    try:
        for t in range(tw.c.steps):
            if t == RESTART_AT:
                tw.reset(RESTART_ENVS)
            tw.step()
        tw.finish()
    finally:
        tw.close()


@pytest.mark.parametrize("name", jc.WORLD_CASES)
def test_world_and_observation_code_objects(name, compiled):
    tw = jc.Twin(jc.case(name), jc.E_MATRIX, "sync")
    try:
        eng = tw.spec
        assert not eng.jit_pending()
        got = (eng.handler_variant, eng.world_variant, eng.obs_variant)
        if name in jc.WORLD_REFUSED:
            # a world kernel of more than 64 KiB of LDS: the code object compiles and is refused, the generic kernel stays
            assert [k for k, _ in eng.jit_errors] == ["world"] and jc.LDS_REFUSAL.decode() in eng.jit_errors[0][1], eng.jit_errors
            assert tw.plain.paths["world_lds_64k"]
            assert got == (0, 0, 9), got
        else:
            assert eng.jit_errors == [], eng.jit_errors
            # (the rung-3 preset's observation shape keeps the build's instance: no observation code object is asked for)
            assert got == (9, 9, 3 if name in jc.PRESET_OBS else 9), got
        assert (tw.plain.handler_variant, tw.plain.world_variant, tw.plain.obs_variant) == (0, 0, 3 if name in jc.PRESET_OBS else 0)
    except BaseException:
        tw.close()
        raise
    _run(tw)


@pytest.mark.parametrize("name", jc.OBS_CASES)
def test_observation_code_object_alone(name, compiled):
    """The world kernel stays generic.  A shape whose observation kernel needs more than 64 KiB of LDS is refused by
    mgx_attach_code; the engine then keeps its generic kernel and still has to match the twin and the oracle."""
    tw = jc.Twin(jc.case(name), jc.E_MATRIX, "obs")
    try:
        eng = tw.spec
        assert (eng.attach_rc != 0) == (name in jc.OBS_REFUSED), (name, eng.attach_rc, eng.attach_error)
        if eng.attach_rc != 0:
            assert jc.LDS_REFUSAL in eng.attach_error, eng.attach_error
            assert eng.obs_variant == 0
        else:
            assert eng.obs_variant == 9
        # no world code object: the twin's world kernel (map_max_few has the rung-3 preset's handlers, the build's code: 3)
        assert eng.world_variant == 0 and eng.handler_variant == tw.plain.handler_variant != 9
        assert tw.plain.obs_variant == 0
    except BaseException:
        tw.close()
        raise
    _run(tw)
