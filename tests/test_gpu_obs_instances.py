"""GPU: every row of the observation kernel's two instance tables (csrc/mgx_obs_instances.h: the token-row rows of
mgx_engine.hip, the dense-output rows of mgx_obs_box.hip) is launched in both of its forms, so that a mis-keyed or missing
row cannot hide behind scenarios that happen not to reach it.

One case per token-row row, E = 3.  Which row the planner (MgxPlan::size_obs) sends a case to is pinned in CASES and read
back from the engine's verbose create line, so a planner change that moves a case off its row fails here.  Then, per case:
the with-rewards form (a few steps against the oracle), the without-rewards form (the initial observations, and a masked
host restart of env 1 against a freshly created engine), and the dense-output row with the same key in both forms against
the decoded rows of a token engine.  The preset rows (variants 3 and 5) have no dense-output twin: with dense output on
they take the generic lean row, like the plain lean case.

No scenario of helpers.SCENARIOS / LIMIT_SCENARIOS reaches the lean row without the program block in LDS or the 512-thread
rows with 3 and 2 encode wavefronts at E = 3 (rung4_full and agents_ext_max both plan 4), so those three cases are derived:
rung 3 with one more, long reward expression per agent, which pushes the interpreted block past 8 KiB, and the rung-4 rules with
the fewest agents that plan 512 threads (48) on a 20 x 20 map with a token budget of 600 / 800."""
import re

import numpy as np
import pytest

import helpers as hp
import obs_decode
import oracle_py as op
from mettagrid_amd import presets
from mettagrid_amd import spec as S
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_map

pytestmark = pytest.mark.gpu

E = 3
STEPS = 4
ROWS = ("obs", "terminals", "truncations", "rewards")


def _rung3_192(max_steps):
    spec = presets.rung3_spec()
    spec.max_steps = max_steps
    return compile_spec(spec, 32, 32, max_objects=192), presets.rung3_map


def _scenario(name):
    spec_f, map_f, _, _ = hp.scenario(name)
    return hp.compile_scenario(name, spec_f(), *map_f(0).shape), map_f


def _rung3_long_rewards():
    """Rung 3 whose agents each carry one more reward, a 30-term sum of their own: INV_FEATURES..OBS_VALUES no longer fit
    the 8 KiB the lean kernel copies into LDS."""
    spec = presets.rung3_spec()
    res = spec.resource_names
    for i, a in enumerate(spec.agents):
        a.rewards = list(a.rewards) + [S.RewardSpec(S.SumValue([S.InventoryValue(res[j % len(res)]) for j in range(30)],
                                                               weights=[0.001 * (1 + i) * (1 + j % 3) for j in range(30)]))]
    return compile_spec(spec, 32, 32), presets.rung3_map


def _rung4_48(obs_tokens):
    spec = hp.teams_spec(presets.rung4_spec(obs_tokens=obs_tokens), 48, 4)
    spec.obs.width = spec.obs.height = 5   # (crowded: see helpers.ext_agents_spec)
    objs = {k: max(1, v // 8) for k, v in presets.RUNG4_OBJECTS.items()}
    return compile_spec(spec, 20, 20), lambda s: random_map(20, 20, objs, hp.team_counts(48, presets.RUNG4_TEAMS), s)


# case: (program and map factory, the row's key: extended, program block in LDS, threads, encode wavefronts, obs_variant)
CASES = {
    "preset": (lambda: _rung3_192(0), (False, True, 256, 4, 3)),
    "preset_any_length": (lambda: _rung3_192(9), (False, True, 256, 4, 5)),
    "lean": (lambda: _scenario("rung1"), (False, True, 256, 4, 0)),
    "lean_block_in_hbm": (_rung3_long_rewards, (False, False, 256, 4, 0)),
    "extended_256": (lambda: _scenario("lit"), (True, False, 256, 4, 0)),
    "extended_512_ew4": (lambda: _scenario("rung4_full"), (True, False, 512, 4, 0)),
    "extended_512_ew3": (lambda: _rung4_48(600), (True, False, 512, 3, 0)),
    "extended_512_ew2": (lambda: _rung4_48(800), (True, False, 512, 2, 0)),
}


def _rows(eng):
    eng.sync()
    return {k: getattr(eng, k).copy().reshape((E, eng.A) + getattr(eng, k).shape[1:]) for k in ROWS}


@pytest.mark.parametrize("case", list(CASES))
def test_every_instance_row_in_both_forms(case, monkeypatch, capfd):
    import torch
    make, key = CASES[case]
    prog, map_f = make()
    A = prog.num_agents
    cms = np.stack([prog.class_map(map_f(s)) for s in range(E)])
    seeds = np.arange(E, dtype=np.uint32) * 7 + 3
    acts = [hp.make_actions(prog, i, STEPS, False) for i in range(E)]
    joint = [(np.concatenate([acts[i][0][t] for i in range(E)]), np.concatenate([acts[i][1][t] for i in range(E)])) for t in range(STEPS)]

    # ---- the row this case is pinned to ----
    capfd.readouterr()
    monkeypatch.setenv("MGX_VERBOSE", "1")
    eng = BatchedMettaGrid(prog, cms, seeds, buffers="host")
    monkeypatch.delenv("MGX_VERBOSE")
    line = re.search(r"\[mgx\] obs: .* blk_lds=(\d) .* threads=(\d+) encode wavefronts=(\d+)", capfd.readouterr().err)
    assert line, "no verbose create line of the observation kernel"
    x = bool(eng.paths["X"])
    got = (x, not x and line.group(1) == "1", int(line.group(2)), int(line.group(3)), eng.obs_variant)
    assert got == key, f"{case}: the planner now sends this case to {got}, not to {key}; pick another program for the row"
    engines = [eng]
    try:
        # ---- token rows: initial observations (without rewards, all envs) and steps (with rewards) against the oracle ----
        oracles = {i: op.OracleSim(prog, cms[i], int(seeds[i])) for i in (0, E - 1)}
        for o in oracles.values():
            o.reinit_buffers()
        for t in range(STEPS + 1):
            snap = eng.snapshot()
            for i, o in oracles.items():
                hp.compare_snapshots(o.snapshot(), {k: v[i * A:(i + 1) * A] for k, v in snap.items()}, f"{case} env {i} step {t}")
            if t == STEPS:
                break
            eng.actions[:], eng.vibe_actions[:] = joint[t]
            eng.step()
            for i, o in oracles.items():
                o.step(acts[i][0][t], acts[i][1][t])
        assert eng.poll_errors()[0] == 0

        # ---- token rows, without rewards, masked: env 1 restarts on env 2's map (no larger token pool: the row stays) ----
        mask = np.array([0, 1, 0], np.uint8)
        new_cms, new_seeds = np.roll(cms, -1, axis=0), seeds + 100
        fresh = BatchedMettaGrid(prog, new_cms, new_seeds, buffers="host")
        engines.append(fresh)
        before = _rows(eng)
        eng.reset_envs(mask, new_cms, new_seeds)
        after, want = _rows(eng), _rows(fresh)
        for k in ROWS:
            assert np.array_equal(after[k][1], want[k][1]), f"{case}: restarted env, '{k}' differs from a fresh engine"
            assert np.array_equal(after[k][[0, 2]], before[k][[0, 2]]), f"{case}: '{k}' of an env that was not restarted changed"

        # ---- dense output: the box row with the same key, both forms, against the decoded rows of a token engine ----
        C, H, W = len(prog.feature_norms), int(prog.words[13]), int(prog.words[14])   # MGX_H_OBS_HEIGHT / WIDTH
        scale = obs_decode.feature_scale(prog.feature_norms)
        tok = BatchedMettaGrid(prog, cms, seeds, buffers="device")
        box_eng = BatchedMettaGrid(prog, cms, seeds, buffers="device")
        engines += [tok, box_eng]
        box = torch.full((E * A, C, H, W), 7.0, dtype=torch.float32, device="cuda")
        box_eng.set_box_output(box)

        def same(what):
            for e in (tok, box_eng):
                e.sync()
            torch.cuda.synchronize()
            want = obs_decode.decode(tok.obs.cpu().numpy(), C, H, W, scale)
            assert np.array_equal(box.cpu().numpy(), want), f"{case}: dense output differs from the decoded token rows {what}"
            assert torch.equal(box_eng.rewards, tok.rewards)

        for t in range(2):
            for e in (tok, box_eng):
                e.actions.copy_(torch.from_numpy(joint[t][0]))
                e.vibe_actions.copy_(torch.from_numpy(joint[t][1]))
            torch.cuda.synchronize()
            for e in (tok, box_eng):
                e.step()
            same(f"after step {t + 1}")
        for e in (tok, box_eng):
            e.reset_envs(mask, new_cms, new_seeds)
        same("after the restart of env 1")
        assert box_eng.poll_errors()[0] == 0
    finally:
        for e in engines:
            e.close()
