"""GPU: the dispatch records (csrc/mgx_world.h MgxDispatchRecs, tests/test_gpu_dispatch_records.py) in a run-time specialised world
kernel: a program other than the preset.  Sorted behind the other run-time specialisation tests, which have compiled the case
table by then (tests/jit_cases.py: one cache per test process)."""
import os

import pytest

import jit_cases as jc

pytestmark = pytest.mark.gpu
NO_GEN, NO_MF, COUNT = "MGX_NO_GEN", "MGX_NO_MOVE_FAST", "MGX_MOVE_FAST_COUNT"
E45 = 45


def _twin_under(c, tw, switch):
    os.environ[switch] = "1"
    try:
        return jc.engine(c, tw.cms, tw.seeds, False)
    finally:
        del os.environ[switch]


def test_run_time_specialised_kernel_at_the_inventory_ceiling():
    """`ceiling_b10` of tests/jit_cases.py through its run-time specialised world kernel (handler and world variant 9, the
    default move's handler table — MgxDev::move_fast on, the one shape under which do_move fills the records): four agents on
    7x8 among vaults and sinks, transfers and deltas into inventories that stand at their limit of 65 535 (free_space returns 0,
    the update clamps, limits with modifiers), beside the generic twin, the oracle, a twin on the interpreter and a twin
    without run-ahead.  At least one action in four takes the general path (the engine's run-ahead counters; the oracle's
    state in front of every step shows an object with on_use ahead of 0.298 of the actions on envs 0, 31, 32, 44)."""
    c = jc.case("ceiling_b10")
    jc.wait_for(labels=("ceiling_b10",))
    with jc.cache_env():
        os.environ[COUNT] = "1"
        try:
            tw = jc.Twin(c, E45, "sync")
        finally:
            del os.environ[COUNT]
        interp = slow = None
        try:
            assert (tw.spec.handler_variant, tw.spec.world_variant) == (9, 9) and tw.spec.jit_errors == []
            assert tw.spec.move_fast in (1, 3) and tw.spec.dispatch_pairs == 1, (tw.spec.move_fast, tw.spec.dispatch_pairs)
            interp = _twin_under(c, tw, NO_GEN)
            assert interp.handler_variant == 0 and interp.world_variant == 0
            slow = _twin_under(c, tw, NO_MF)
            assert slow.move_fast == 0 and slow.world_variant == 0
            for t in range(c.steps):
                tw.step(extra=(interp, slow))
                stat_envs = tw.envs if t % 10 == 9 or t == c.steps - 1 else ()
                jc.same_everywhere(tw.spec, interp, f"specialised vs interpreter twin, step {t + 1}", stat_envs)
                jc.same_everywhere(tw.spec, slow, f"specialised vs twin without run-ahead, step {t + 1}", stat_envs)
            tw.finish()
            ran, _ = tw.spec.move_fast_counts()
            total = E45 * tw.A * c.steps
            share = (total - ran) / total
            print(f"general path: {total - ran} of {total} actions ({share:.3f})")
            assert share >= 0.25, f"only {share:.3f} of the actions took the general path"
        finally:
            for g in (interp, slow):
                if g is not None:
                    g.close()
            tw.close()
