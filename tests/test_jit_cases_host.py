"""CPU: what the run-time specialisation tests (tests/jit_cases.py) cover, pinned where no GPU is needed: the spread of the
planner's decisions over the world cases (a folded shape takes the branches the planner chose, so a branch no case's
planner result takes is compiled by nothing), what `jit.plan` hands the compiler, and the generated handler header."""
import re

import pytest

import jit_cases as jc
from mettagrid_amd import engine, gen_handlers, gen_presets, jit
from mettagrid_amd.fmt import K


@pytest.fixture(scope="module")
def fields():
    """{world case: {field: value}} from the library's host-only planner query, create-time switches at their defaults."""
    import os
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("MGX_")]}
    try:
        lib = engine.load_lib()
        return {n: dict(zip(gen_presets.WORLD_FIELDS, gen_presets.world_fields_of(jc.case(n).prog, lib))) for n in jc.WORLD_CASES}
    finally:
        os.environ.update(saved)


def _spread(fields, f):
    return {n: v[f] for n, v in fields.items()}


@pytest.mark.parametrize("field", ["duo", "tick_split", "any_on_tick", "defer_book"])
def test_planner_switch_takes_both_values(fields, field):
    got = _spread(fields, field)
    assert set(got.values()) == {0, 1}, got


def test_booked_mid_is_the_case_that_books_every_action_as_it_happens(fields):
    assert fields["booked_mid"]["defer_book"] == 0 and fields["tags"]["defer_book"] == 1, _spread(fields, "defer_book")


def test_move_handler_count_and_game_stat_sets_spread(fields):
    nm, ng = _spread(fields, "n_move_handlers"), _spread(fields, "act_ngset")
    assert set(nm.values()) == {2, 3}, nm
    assert nm["ranged"] == 3
    assert 0 in ng.values() and any(v > 0 for v in ng.values()), ng


def test_move_fast_fields_spread(fields):
    """`move_fast` (0: every move takes the general path; 1: relocate + use, the reference's default move table), `mf_exact`
    (1: an exact bitmap of the map; 0: the hashed mask of maps above 1 024 cells or where the bitmap would cost a workgroup
    per CU) and `shadow` (3: integer bookkeeping; 0: none) as the real library decides them.

    Where a value cannot be reached by a lean program of this table, and why:
      * move_fast = 3 needs a move table of ONE handler (relocate only); every case keeps the default use handler, so the
        values here are 0 and 1.
      * shadow = 1 (counters without coverage stats) exists only under the lane-per-agent dispatch, which lean programs take
        on request only (MGX_ACT_LEAN); a lean program's planner result is 0 or 3."""
    for f in ("move_fast", "mf_exact", "shadow"):
        print(f, _spread(fields, f))
    mf = _spread(fields, "move_fast")
    assert {0, 1} <= set(mf.values()), mf
    assert mf["ranged"] == 0 and mf["booked_mid"] == 0        # a ranged handler / no deferred bookkeeping: no run-ahead
    exact = {n: fields[n]["mf_exact"] for n in fields if mf[n]}   # (the field means something only where move_fast is on)
    assert set(exact.values()) == {0, 1}, exact
    assert exact["hashed"] == 0 and fields["hashed"]["mf_dirty_words"] == 4
    sh = _spread(fields, "shadow")
    assert set(sh.values()) == {0, 3}, sh


def test_every_world_case_is_lean_and_not_a_build_time_preset(fields):
    presets_obs = gen_presets.preset_shapes()
    for n in jc.WORLD_CASES + jc.OBS_CASES:
        sh = gen_presets.shape_of(jc.case(n).prog)
        assert not sh["extended"], n
        # a preset's observation shape: the engine keeps the build's instance (obs_variant 3 / 5) and asks for no code object
        preset = [name for name, p in presets_obs.items() if all(sh[f] == p[f] for f in gen_presets.FIELDS if f != "MAX_STEPS")]
        assert preset == (["R3"] if n in jc.PRESET_OBS else []), (n, preset)
    for n, v in fields.items():
        assert v["gen_prog"] == 0, (n, v["gen_prog"])
        assert v["coop_passes"] == 1, n


def test_plan_gives_world_and_obs_with_the_planners_shape(fields, monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("MGX_")]:   # (the planner was asked under the default switches: `fields`)
        monkeypatch.delenv(k)
    monkeypatch.setenv("MGX_JIT_CACHE", jc.cache())
    keys = {}
    for n in jc.WORLD_CASES:
        plan = jit.plan(jc.case(n).prog)
        assert sorted(plan) == ["obs", "world"], (n, sorted(plan))
        obj, argv, gen = plan["world"]
        assert obj.startswith(jc.cache()) and gen is not None
        define = [a for a in argv if a.startswith("-DMGX_JIT_WORLD_SHAPE=")]
        assert len(define) == 1, n
        want = dict(fields[n], gen_prog=jit.JIT_GEN_ID)
        assert [int(x) for x in define[0].split("=", 1)[1].split(",")] == [want[f] for f in gen_presets.WORLD_FIELDS], n
        keys[n] = obj
    for a in jc.WORLD_CASES:
        for b in jc.WORLD_CASES:
            if a < b and keys[a] == keys[b]:
                assert any(a in g and b in g for g in jc.SHARED_WORLD), f"{a} and {b} share {keys[a]}"
    for n in jc.OBS_CASES:
        assert "obs" in jit.plan(jc.case(n).prog), n


def _reachable(prog) -> set:
    """Handler ids reachable from the move handlers, the classes' on_use / on_after_use / on_tick hooks and the game's on_tick."""
    p = gen_handlers._Prog(prog)
    todo = [m[K.MH_HANDLER] for m in p.move] + [h for hooks in p.class_hooks for h in hooks] + [p.game_on_tick]
    seen = set()
    while todo:
        h = todo.pop()
        if h < 0 or h in seen:
            continue
        seen.add(h)
        hd = p.handlers[h]
        if hd[K.HD_KIND] != K.HK_LEAF:
            todo += p.children[hd[K.HD_CHILD_START]: hd[K.HD_CHILD_START] + hd[K.HD_CHILD_COUNT]]
    return seen


@pytest.mark.parametrize("name", jc.WORLD_CASES)
def test_generated_header_has_a_function_for_every_reachable_handler(name):
    prog = jc.case(name).prog
    lines, fp = gen_handlers.render_one("J", prog)
    assert fp != 0, f"{name}: no generated code (a handler nests deeper than the register VM's frames?)"
    text = "\n".join(lines)
    defined = {int(h) for h in re.findall(r"bool h(\d+)_L\d+\(", text)}
    want = _reachable(prog)
    assert want and want <= defined, (name, sorted(want - defined))


def test_nest4_lean_fills_the_register_vms_frames():
    """The deepest call chain of `nest4_lean` — a move handler, UseTarget, an on_use tree of three levels — needs exactly the
    four frames run_handler has, and the generator still renders it (one more level and render_one gives up: fingerprint 0)."""
    p = gen_handlers._Prog(jc.case("nest4_lean").prog)
    use_roots = [h for u, a, _ in p.class_hooks for h in (u, a) if h >= 0]

    def frames(h, used):
        hd = p.handlers[h]
        if hd[K.HD_KIND] != K.HK_LEAF:
            return 1 + max(frames(k, used) for k in p.children[hd[K.HD_CHILD_START]: hd[K.HD_CHILD_START] + hd[K.HD_CHILD_COUNT]])
        if gen_handlers._uses_target(p, [h]) and not used:
            return 1 + max(frames(k, True) for k in use_roots)
        return 1

    assert max(frames(m[K.MH_HANDLER], False) for m in p.move) == gen_handlers.MAX_FRAMES == 4
    assert gen_handlers._levels(p) is not None
    import helpers as hp
    from mettagrid_amd.compiler import compile_spec
    deeper = compile_spec(hp.nesting_spec(4, extended=False), 9, 9)
    assert gen_handlers.render_one("J", deeper)[1] == 0


# ---- the runner's action streams on the oracle, all 45 envs ---------------------------------------------------------------------
@pytest.mark.parametrize("name", jc.WORLD_CASES + jc.OBS_CASES)
def test_no_env_of_a_case_raises_an_error_bit(name):
    """The GPU runner requires the engines' error bits (all envs) to equal the oracles' (four envs), so no env may raise one:
    the matrix's run of every case — stream, maps, masked restart — on 45 oracles.  A token overflow in particular is an
    error in the reference, and what the engines do past one is defined by nothing."""
    c = jc.case(name)
    bits, fullest = jc.oracle_sweep(c, jc.E_MATRIX, c.steps, restart_at=jc.RESTART_AT, restart_envs=jc.RESTART_ENVS)
    assert bits == 0, (name, bits)
    assert fullest <= c.prog.num_tokens
    if name == "window15":   # the case that is there for the full budget: the last token in the last slot, and not one more
        assert fullest == c.prog.num_tokens == 185


@pytest.mark.parametrize("name", ["torture", "window15"])
def test_no_env_raises_an_error_bit_in_the_paths_runs(name):
    """... and the runs of tests/test_gpu_jit_paths.py that an oracle can follow: 33 steps without a restart (the attach in
    mid-episode; the rebinding and dense-output runs are its first steps) and the restart onto denser maps."""
    import numpy as np
    c = jc.case(name)
    assert jc.oracle_sweep(c, jc.E_MATRIX, 33)[0] == 0
    sparse = np.stack([c.prog.class_map(jc.SPARSE[name](s)) for s in range(jc.E_MATRIX)])
    dense = [c.prog.class_map(jc.DENSE[name](700 + k)) for k in range(len(jc.DENSE_ENVS))]
    bits, _ = jc.oracle_sweep(c, jc.E_MATRIX, jc.DENSE_STEPS, cms=sparse, restart_at=jc.DENSE_AT, restart_envs=jc.DENSE_ENVS, restart_maps=dense)
    assert bits == 0
    if name == "torture":   # the second engine of test_two_specialised_engines_of_one_program_alive_at_once
        assert jc.oracle_sweep(c, jc.E_MATRIX, 20, action_seed=99, seed0=1001, cms=jc.class_maps(c, range(300, 300 + jc.E_MATRIX)))[0] == 0


def test_cleanup_stops_a_running_compiler_and_its_children(tmp_path, monkeypatch):
    """What jit_cases registers at exit, on a live job: a stand-in for hipcc that starts a child and waits for it."""
    import subprocess
    import sys
    import time
    script = "import subprocess, sys; p = subprocess.Popen([sys.executable, '-c', 'import time; print(1, flush=True); time.sleep(60)'], " \
             "stdout=subprocess.PIPE); print(p.pid, flush=True); p.stdout.readline(); print('up', flush=True); p.wait()"
    proc = subprocess.Popen([sys.executable, "-c", script], stdout=subprocess.PIPE, text=True)
    child = int(proc.stdout.readline())
    assert proc.stdout.readline().strip() == "up"
    job = jit.Job("world", str(tmp_path / "x.hsaco"), proc, str(tmp_path / "x.log"))
    monkeypatch.setattr(jc, "_jobs", {("stand-in", "world"): job})
    assert sorted(jc._descendants(proc.pid)) == sorted([proc.pid, child])
    jc._stop_compilers()
    assert proc.poll() is not None
    for _ in range(50):   # (the child is no child of this process: it is reaped by init a moment after the signal)
        try:
            state = open(f"/proc/{child}/stat").read().rsplit(")", 1)[1].split()[0]
        except OSError:
            state = "gone"
        if state in ("gone", "Z"):
            break
        time.sleep(0.1)
    assert state in ("gone", "Z"), state
