"""Cases of the run-time specialisation tests (mettagrid_amd/jit.py + mgx_attach_code): the programs whose code objects
tests/test_gpu_jit.py, tests/test_gpu_jit_matrix.py and tests/test_gpu_jit_paths.py run, one cache directory per test
process that all of them share, `start_all()` that compiles every code object once and side by side, and the runner that
steps a specialised engine beside a `specialize=False` twin and the oracle.  tests/test_jit_cases_host.py pins, without a
GPU, what the planner decides for these programs.  No tests here."""
from __future__ import annotations

import atexit
import collections
import contextlib
import copy
import json
import os
import shutil
import tempfile
import time

import numpy as np

import helpers as hp
from mettagrid_amd import jit, presets
from mettagrid_amd import spec as S
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.mapgen import random_map

HERE = os.path.dirname(os.path.abspath(__file__))

# World + observation code objects (12 cases; 11 world code objects run: WORLD_REFUSED below).  The order is the order of the compile queue's long units and of the list a slow
# machine drops from (from the end of the scenario names: crowd, keyhole, tags).
WORLD_CASES = ("torture", "minmax", "thirteen", "rung3_flat_damage", "ceiling_b10", "tags", "nest4_lean", "keyhole", "crowd",
               "ranged", "booked_mid", "hashed")
# Observation code object only: the world kernel stays generic.
OBS_CASES = ("wide", "letterbox", "window15", "agents_lean_max", "torture_base10", "torture_terminal", "ceiling_b2", "ceiling_b256",
             "map_max_few")
# World cases that may share one world code object (same generated text, fingerprint and folded shape): none today.
SHARED_WORLD = ()
MAX_STEPS = 40          # a case runs its scenario's own step count, capped
MAX_COMPILERS = 16      # hipcc processes alive at a time
E_MATRIX = 45           # one full wavefront of 32 envs (MGX_WORLD_LPW) and one of 13
LDS_REFUSAL = b"more than 64 KiB of LDS"

# Cases whose engine keeps the interpreted program in global memory (tests/test_gpu_paths.py EXPECTED: no 'prog_lds'): the
# world unit is compiled for that form, as the engine will ask for it.
PROG_NOT_IN_LDS = ("crowd", "agents_lean_max")
# World cases whose world kernel needs more than 64 KiB of LDS (EXPECTED: 'world_lds_64k'; 70 agents x 64 envs per workgroup):
# mgx_attach_code refuses the world code object and the engine keeps its generic world kernel.
WORLD_REFUSED = ("crowd",)
# Observation cases at a capacity limit of the observation kernel's LDS staging (helpers.LIMIT_SCENARIOS: the most agents, the
# largest map; up to 160 KiB): more than the 64 KiB a code object's kernel may ask for, so mgx_attach_code refuses it.
OBS_REFUSED = ("agents_lean_max", "map_max_few")
# World cases whose observation shape is the rung-3 preset's: the engine runs the build's instance (obs_variant 3) and asks
# for no observation code object.
PRESET_OBS = ("ranged",)
# The seed of a case's action stream.  A row that would take one token more than the budget is an error in the reference
# (it raises), so every case runs a stream under which no env of the 45 overflows: tests/test_jit_cases_host.py checks that on
# the oracle for all envs.  Under seed 17 `window15` (rows at the budget) and `thirteen` (13 resources in 120 tokens) overflow
# in a few envs; under 20, window15's fullest row holds exactly its 185 tokens: the last token in the last slot.
ACTION_SEED = 17
ACTION_SEEDS = {"window15": 20, "thirteen": 37}
RESTART_AT, RESTART_ENVS = 10, (1, 32)     # the matrix's masked restart

Case = collections.namedtuple("Case", "name prog map_f steps invalid world prog_lds action_seed")


def ranged_spec() -> S.GameSpec:
    """Rung 3 with a third, ranged move handler (tests/test_gpu_world_shape.py _one_field_off): n_move_handlers = 3 and a
    move handler that looks two cells ahead, so no paired dispatch and no run-ahead of moves."""
    spec = copy.deepcopy(presets.rung3_spec())
    spec.move_handlers = [S.Handler([S.VibeFilter(S.ACTOR, "b"), S.MaxDistanceFilter(S.TARGET, 2), S.TargetIsUsableFilter()],
                                    [S.UseTarget()], "reach")]
    return spec


def ranged_map(seed: int) -> np.ndarray:
    return random_map(32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, 900 + seed)


def booked_mid_spec() -> S.GameSpec:
    """The `tags` rules with one filter that reads a per-action bookkeeping counter in the middle of a tick: the planner then
    has to book every action as it happens (MgxDev::defer_book = 0, csrc/mgx_plan.h) instead of at the end of the launch."""
    sp = hp.tags_spec()
    A = S.ACTOR
    walked = S.Handler([S.GameValueFilter(A, S.StatValue("action.move.success", "agent"), S.ConstValue(3.0))],
                       [S.ResourceDelta(A, "gem", 1)], "walked")
    post = sp.objects["post"]
    post.on_use = S.FirstMatch([walked] + list(post.on_use.handlers))
    return sp


def hashed_map(seed: int) -> np.ndarray:
    """The `ceiling` cells on a map of more than 1 024 cells: the run-ahead of moves then keeps a hashed mask of the map in LDS
    instead of an exact bitmap (MgxDev::mf_exact = 0 with move_fast on, csrc/mgx_plan.h)."""
    return random_map(33, 32, {"wall": 24, "vault": 14, "sink": 12}, 4, seed)


_CUSTOM = {
    "ranged": (ranged_spec, ranged_map, MAX_STEPS, True),
    "booked_mid": (booked_mid_spec, hp.tags_map, MAX_STEPS, True),
    "hashed": (lambda: hp.ceiling_spec(10), hashed_map, MAX_STEPS, True),
}
MAX_OBJECTS = dict(hp.MAX_OBJECTS, ranged=192)
_cases: dict = {}


def case(name: str) -> Case:
    """The case table's row of ``name`` (compiled once per process)."""
    if name not in _cases:
        spec_f, map_f, steps, invalid = _CUSTOM[name] if name in _CUSTOM else hp.scenario(name)
        h, w = map_f(0).shape
        prog = compile_spec(spec_f(), h, w, max_objects=MAX_OBJECTS.get(name))
        _cases[name] = Case(name, prog, map_f, min(steps, MAX_STEPS), invalid, name in WORLD_CASES, name not in PROG_NOT_IN_LDS,
                             ACTION_SEEDS.get(name, ACTION_SEED))
    return _cases[name]


def class_maps(c: Case, seeds) -> np.ndarray:
    return np.stack([c.prog.class_map(c.map_f(int(s))) for s in seeds])


# ---- the programs tests/test_gpu_jit.py compiles beside the table's ---------------------------------------------------------
def reference_programs() -> list:
    """(name, program, map) of the reference's arena and navigation configs (fixtures of its own converter)."""
    import ref_tree
    from mettagrid_amd import from_reference
    out = []
    for name in ("arena", "navigation"):
        doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
        prog = from_reference.compile_reference_config(ref_tree.load(doc["config"]), len(doc["map"]), len(doc["map"][0]))
        out.append((name, prog, doc["map"]))
    return out


def extended_programs() -> list:
    """The two extended programs whose dispatch kernel tests/test_gpu_jit.py specialises: a rung-4 game whose chests mark a
    game stat, and the reference's handler-chain config."""
    import ref_tree
    from mettagrid_amd import from_reference
    spec = presets.rung4_spec(obs_tokens=400)
    spec.objects["chest"].on_use = S.Handler([S.ResourceFilter(S.ACTOR, "ore", 2)],
                                             [S.ResourceTransfer(S.ACTOR, S.TARGET, "ore", -2),
                                              S.SetStat("chest.ore", S.InventoryValue("ore"), scope="game", entity=S.TARGET)], "deposit2")
    prog = compile_spec(spec, 20, 20, max_objects=presets.RUNG4_MAX_OBJECTS)
    doc = json.load(open(os.path.join(HERE, "golden", "ref_chains.json")))
    chains = from_reference.compile_reference_config(ref_tree.load(doc["config"]), len(doc["map"]), len(doc["map"][0]))
    return [("rung4_deposit2", prog), ("ref_chains", chains)]


# ---- one cache per test process -----------------------------------------------------------------------------------------------
_cache = None
_jobs = None


def _descendants(pid: int) -> list:
    """``pid`` and the processes below it (hipcc starts the compiler proper as children), from /proc."""
    kids: dict = {}
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                stat = open(f"/proc/{d}/stat").read()
                kids.setdefault(int(stat[stat.rindex(")") + 2:].split()[1]), []).append(int(d))
            except (OSError, ValueError, IndexError):
                pass
    out, todo = [], [pid]
    while todo:
        q = todo.pop()
        out.append(q)
        todo += kids.get(q, [])
    return out


def _stop_compilers() -> None:
    """End the compilers that are still running, children included.  (Reads jit.Job's process handle, which has no public
    name; tests/test_jit_cases_host.py runs this on a live job, so a rename there fails a test instead of disarming this.)"""
    import signal
    for j in (_jobs or {}).values():
        proc = j._proc
        if proc is not None and proc.poll() is None:
            for pid in _descendants(proc.pid):
                try:
                    os.kill(pid, signal.SIGTERM)
                except OSError:
                    pass
            try:
                proc.wait(10)
            except Exception:
                proc.kill()


def _cleanup() -> None:
    """At exit: stop what is still compiling (a session that selected one test, or one that failed early), then remove the
    cache directory."""
    _stop_compilers()
    if _cache is not None:
        shutil.rmtree(_cache, True)


def cache() -> str:
    """The code-object cache of this test process: a fresh temporary directory, removed at exit.  The in-tree cache is never
    used, so that a stale object cannot hide a failed compile."""
    global _cache
    if _cache is None:
        _cache = tempfile.mkdtemp(prefix="mgx_jit_tests_")
        atexit.register(_cleanup)
    return _cache


@contextlib.contextmanager
def cache_env():
    """MGX_JIT_CACHE = `cache()` inside the block: what every user of the table runs its compiles and engines under."""
    old = os.environ.get("MGX_JIT_CACHE")
    os.environ["MGX_JIT_CACHE"] = cache()
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MGX_JIT_CACHE", None)
        else:
            os.environ["MGX_JIT_CACHE"] = old


def _units() -> list:
    """(label, program, kind, program in LDS) of every code object, the long units (world, dispatch) first."""
    long_units = [(n, case(n).prog, "world", case(n).prog_lds) for n in WORLD_CASES]
    refs = reference_programs()
    long_units += [(n, p, "world", True) for n, p, _ in refs]
    long_units += [(n, p, "actx", True) for n, p in extended_programs()]
    short = [(n, case(n).prog, "obs", True) for n in WORLD_CASES + OBS_CASES if n not in PRESET_OBS] + [(n, p, "obs", True) for n, p, _ in refs]
    return long_units + short


def start_all() -> dict:
    """Start every code object of the table (and of tests/test_gpu_jit.py) once per process, into `cache()`: {(label, kind):
    Job}.  At most MAX_COMPILERS compilers are alive at a time: the long units go first and all together, the observation
    units (seconds each) take turns on what is left.  Compilers still running when the process ends are stopped (_cleanup)."""
    global _jobs
    if _jobs is not None:
        return _jobs
    with cache_env():
        _jobs, alive = {}, []     # (filled as it goes: _cleanup finds what was started even if this raises)
        for label, prog, kind, pl in _units():
            alive = [j for j in alive if not j.ready()]
            while len(alive) >= MAX_COMPILERS:
                time.sleep(0.2)
                alive = [j for j in alive if not j.ready()]
            got = jit.start(prog, pl, kinds=(kind,))
            assert len(got) == 1 and got[0].kind == kind, (label, kind, [j.kind for j in got])
            _jobs[(label, kind)] = got[0]
            alive.append(got[0])
    return _jobs


def wait_for(labels=None, timeout: float = 900) -> dict:
    """Wait for the jobs of ``labels`` (all: None); every one must have compiled."""
    jobs = {k: j for k, j in start_all().items() if labels is None or k[0] in labels}
    for key, j in jobs.items():
        assert j.wait(timeout), f"{key}: still compiling after {timeout} s"
        assert j.error is None, (key, j.error)
    return jobs


# ---- the runner ---------------------------------------------------------------------------------------------------------------
def engine(c: Case, cms, seeds, specialize):
    """A device-buffer engine of a case: ``specialize`` False (the twin), "sync" (world + observation code objects from the
    cache) or "obs" (only the observation code object, attached by hand; a refusal is returned instead of raised)."""
    from mettagrid_amd.engine import BatchedMettaGrid
    if specialize != "obs":
        return BatchedMettaGrid(c.prog, cms, seeds, buffers="device", specialize=specialize)
    eng = BatchedMettaGrid(c.prog, cms, seeds, buffers="device", specialize=False)
    attach_obs(eng, c)
    return eng


def attach_obs(eng, c: Case) -> int:
    """Hand the case's observation code object to a running engine (mgx_attach_code); the return code, with the refusal's
    text in ``eng.attach_error``."""
    job = start_all()[(c.name, "obs")]
    assert job.wait(900) and job.error is None, job.error
    eng.attach_rc = eng.L.mgx_attach_code(eng.h, jit.KINDS["obs"], job.path.encode())
    eng.attach_error = eng.L.mgx_last_error() if eng.attach_rc else b""
    return eng.attach_rc


class Actions:
    """Seeded action streams for E envs: two thirds moves, the rest uniform; ids from [-1, n_act] where invalid ids are allowed."""

    def __init__(self, prog, E: int, seed: int, invalid: bool) -> None:
        self.rng = np.random.default_rng(seed)
        self.n = E * prog.num_agents
        n_act = len(prog.action_names)
        self.lo, self.hi = (-1, n_act + 1) if invalid else (0, n_act)
        self.moves = np.array([i for i, nm in enumerate(prog.action_names) if nm.startswith("move")], dtype=np.int32)

    def next(self) -> tuple:
        rng = self.rng
        a = rng.integers(self.lo, self.hi, self.n).astype(np.int32)
        mv = rng.random(self.n) < 2 / 3
        a[mv] = self.moves[rng.integers(0, len(self.moves), int(mv.sum()))]
        return a, rng.integers(self.lo, self.hi, self.n).astype(np.int32)


def step_engines(engines, a, v) -> None:
    """One step of every engine on the same actions (the engines run on their own streams: ordered behind the writes and back)."""
    import torch
    ta, tv = torch.from_numpy(a).cuda(), torch.from_numpy(v).cuda()
    for e in engines:
        e.actions.copy_(ta); e.vibe_actions.copy_(tv)
        e.wait_for_caller(); e.step(); e.caller_waits()
    torch.cuda.synchronize()


def same_everywhere(x, y, where: str, stat_envs=()) -> None:
    """Two engines of one program agree on every env: state digests, observations, rewards, terminals, truncations,
    action_success, executed actions; every stat row of ``stat_envs``."""
    import torch
    bad = np.nonzero(x.state_digests() != y.state_digests())[0]
    assert len(bad) == 0, f"{where}: digests of envs {bad[:8].tolist()} differ ({len(bad)})"
    torch.cuda.synchronize()
    for k in ("obs", "rewards", "terminals", "truncations"):
        if not torch.equal(getattr(x, k), getattr(y, k)):
            rows = torch.nonzero((getattr(x, k) != getattr(y, k)).reshape(x.E * x.A, -1).any(dim=1)).flatten()[:8].tolist()
            raise AssertionError(f"{where}: '{k}' differs in rows {rows} (env = row // {x.A})")
    assert np.array_equal(x.action_success(), y.action_success()), f"{where}: action_success"
    assert np.array_equal(x.executed_actions(), y.executed_actions()), f"{where}: executed actions"
    assert np.array_equal(x.episode_rewards(), y.episode_rewards()), f"{where}: episode rewards"
    for i in stat_envs:
        for p, q in zip(x.raw_stats(i), y.raw_stats(i)):
            assert np.array_equal(p, q), f"{where}: stats of env {i} differ"


def oracle_sweep(c: Case, E: int, steps: int, action_seed=None, cms=None, seed0: int = 3, restart_at=None, restart_envs=(),
                 restart_maps=None) -> tuple:
    """What a Twin run does, on the oracle alone and for ALL envs (no GPU): (error bits of all envs and episodes, the most
    tokens any row held).  Same maps, seeds, action stream and masked restart as Twin / Twin.reset."""
    import oracle_py as op
    A = c.prog.num_agents
    cms = class_maps(c, range(E)) if cms is None else cms
    seeds = np.arange(E, dtype=np.uint32) * 7 + seed0
    sims = [op.OracleSim(c.prog, cms[i], int(seeds[i])) for i in range(E)]
    for o in sims:
        o.reinit_buffers()
    acts = Actions(c.prog, E, c.action_seed if action_seed is None else action_seed, c.invalid)
    bits = fullest = 0
    for t in range(steps):
        if t == restart_at:
            for k, i in enumerate(restart_envs):
                bits |= int(sims[i].error)
                cm = c.prog.class_map(c.map_f(500 + k)) if restart_maps is None else restart_maps[k]
                sims[i] = op.OracleSim(c.prog, cm, 1000 + 13 * k)
                sims[i].reinit_buffers()
        a, v = acts.next()
        for i, o in enumerate(sims):
            o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
            fullest = max(fullest, int((o.snapshot()["obs"][:, :, 0] != 0xFF).sum(axis=1).max()))
    for o in sims:
        bits |= int(o.error)
    return bits, fullest


# Maps of tests/test_gpu_jit_paths.py's restart onto denser maps: few objects at create, more at the restart (window15: fewer
# than the scenario's own maps, which sit at the token budget).
DENSE = {"torture": lambda s: random_map(12, 14, {"wall": 2, "block": 2, "mine": 14, "forge": 12, "shrine": 12}, {"red": 3, "blue": 3}, s),
         "window15": lambda s: random_map(14, 14, {"wall": 30, "extractor": 8, "chest": 5}, {"red": 6, "blue": 6}, s)}
SPARSE = {"torture": lambda s: random_map(12, 14, {"wall": 14, "block": 8, "mine": 1, "forge": 1, "shrine": 1}, {"red": 3, "blue": 3}, s),
          "window15": lambda s: random_map(14, 14, {"wall": 40, "extractor": 2, "chest": 1}, {"red": 6, "blue": 6}, s)}
DENSE_ENVS, DENSE_AT, DENSE_STEPS = (1, 31, 32, 44), 5, 17


def oracle_envs(E: int) -> list:
    """Both sides of the wavefront boundary and both ends: 0, 31, 32, E - 1 (fewer where E is small)."""
    return sorted({i for i in (0, 31, 32, E - 1) if 0 <= i < E})


class Twin:
    """A specialised engine (`spec`) and its `specialize=False` twin (`plain`) on the same maps, seeds and actions, with the
    oracle on `oracle_envs(E)`: step() steps all of them and compares after the step, finish() compares the signature
    payloads and the error bits."""

    def __init__(self, c: Case, E: int, specialize, action_seed=None, with_oracle: bool = True, cms=None, seed0: int = 3) -> None:
        import oracle_py as op
        self.c, self.E, self.A, self.t = c, E, c.prog.num_agents, 0
        self.cms = class_maps(c, range(E)) if cms is None else np.array(cms)
        self.seeds = np.arange(E, dtype=np.uint32) * 7 + seed0
        self.spec = None
        self.plain = engine(c, self.cms, self.seeds, False)
        try:
            # (else the engine would ask for another world unit than start_all() compiled, and compile it here)
            assert bool(self.plain.L.mgx_world_prog_in_lds(self.plain.h)) == c.prog_lds, f"{c.name}: the program's place is not what the table says"
            self.spec = engine(c, self.cms, self.seeds, specialize)
            self.envs = oracle_envs(E)
            self.oracles, self.since, self.error_bits = {}, {}, 0
            if with_oracle:
                for i in self.envs:
                    self._oracle(op, i)
            self.acts = Actions(c.prog, E, c.action_seed if action_seed is None else action_seed, c.invalid)
            self.check("after create")
        except BaseException:
            self.close()
            raise

    def _oracle(self, op, i: int) -> None:
        if i in self.oracles:
            self.error_bits |= int(self.oracles[i].error)
        self.oracles[i] = op.OracleSim(self.c.prog, self.cms[i], int(self.seeds[i]))
        self.oracles[i].reinit_buffers()
        self.since[i] = self.t

    def check(self, where: str) -> None:
        where = f"{self.c.name} {where}"
        same_everywhere(self.spec, self.plain, where, self.envs)
        if self.oracles:
            snap, A = self.spec.snapshot(), self.A
            for i, o in self.oracles.items():
                hp.compare_snapshots(o.snapshot(), {k: x[i * A:(i + 1) * A] for k, x in snap.items()}, f"{where} env {i} (oracle)")

    def step(self, extra=()) -> tuple:
        a, v = self.acts.next()
        step_engines((self.spec, self.plain) + tuple(extra), a, v)
        A = self.A
        for i, o in self.oracles.items():
            o.step(a[i * A:(i + 1) * A], v[i * A:(i + 1) * A])
        self.t += 1
        self.check(f"step {self.t}")
        return a, v

    def reset(self, envs, map_seed0: int = 500, maps=None) -> None:
        """Masked restart of ``envs`` onto other maps (``maps[k]`` for ``envs[k]``; default: the case's map factory at other
        seeds) and seeds on both engines (oracles of those envs are recreated); every other env must be untouched."""
        import oracle_py as op
        before = self.spec.snapshot()
        digests = self.spec.state_digests()
        mask = np.zeros(self.E, np.uint8)
        mask[list(envs)] = 1
        for k, i in enumerate(envs):
            self.cms[i] = self.c.prog.class_map(self.c.map_f(map_seed0 + k)) if maps is None else maps[k]
            self.seeds[i] = 1000 + 13 * k
        for g in (self.spec, self.plain):
            g.reset_envs(mask, self.cms, self.seeds)
        for i in envs:
            if i in self.oracles:
                self._oracle(op, i)
        self.check(f"after the restart of envs {list(envs)} at step {self.t}")
        after, keep = self.spec.snapshot(), np.repeat(mask == 0, self.A)
        for k in before:
            assert np.array_equal(before[k][keep], after[k][keep]), f"{self.c.name}: the restart touched '{k}' of another env"
        assert np.array_equal(digests[mask == 0], self.spec.state_digests()[mask == 0]), f"{self.c.name}: the restart touched another env's state"

    def finish(self) -> None:
        c, A = self.c, self.A
        bits = self.error_bits
        for o in self.oracles.values():
            bits |= int(o.error)
        (got, first), (got0, first0) = self.spec.poll_errors(), self.plain.poll_errors()
        assert (got, first) == (got0, first0), f"{c.name}: error bits {got} of env {first} (specialised) vs {got0} of env {first0} (generic)"
        # The engines' bits are those of all envs.  With oracles: equal to theirs (the action streams are chosen so that no
        # env of a case raises a bit: ACTION_SEEDS); without: none at all.
        assert got == bits, f"{c.name}: error bits {got} (first env {first}) vs the oracles' {bits}"
        snap = self.spec.snapshot()
        for i, o in self.oracles.items():
            mine = {k: x[i * A:(i + 1) * A] for k, x in snap.items()}
            steps, seed = self.t - self.since[i], int(self.seeds[i])
            pa = hp.payload_from_raw(c.prog, o.raw_objects(), o.current_stat_reward(), o.raw_stats(), o.snapshot(), steps, seed)
            pb = hp.payload_from_raw(c.prog, self.spec.raw_objects(i), self.spec.current_stat_reward(i), self.spec.raw_stats(i), mine, steps, seed)
            assert pa == pb, f"{c.name} env {i}: signature payload differs: {hp.diff_payload(pa, pb)}"

    def close(self) -> None:
        for g in (self.spec, self.plain):
            if g is not None:
                g.close()
