"""Time-averaged game stats against the REFERENCE's own TimeAveragedStatsHandler.  tests/golden/time_avg_<scenario>.json holds
what the handler (python/src/mettagrid/simulator/time_averaged_stats.py:17-41) reported when the reference played the committed
action traces of ref_navigation / ref_chains to the end of the episode, and the reference engine the rung3_s0 golden's trace, in
which a key ("chest.ore") first exists mid-episode (tests/golden/make_time_avg_fixture.py; that trace is 160 steps and stops
before its episode ends, so there the handler's value after 160 steps is what is pinned).  Here: the
oracle replays the trace under the suite's restatement of the handler (``TimeAveragedStats`` below) and must give that dict
key for key and f64 bit for bit — which pins what tests/test_gpu_time_avg.py compares the device accumulation with; on the
GPU the engine's own log record must give it too."""
import json
import os

import numpy as np
import pytest

import helpers as hp
import oracle_py as op
import ref_tree
from mettagrid_amd import from_reference
from mettagrid_amd.signature import stats_dicts

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["navigation", "chains", "rung3_s0"]   # rung3_s0: "chest.ore" first exists when an agent uses the chest


class TimeAveragedStats:
    """The handler restated: on_episode_start zeroes, on_step counts the step and adds every value the game dict holds into a
    Python float, the property divides by the count ({} at zero steps)."""

    def __init__(self) -> None:
        self.step_count = 0
        self.accumulated: dict = {}

    def on_step(self, game: dict) -> None:
        self.step_count += 1
        for key, value in game.items():
            self.accumulated[key] = self.accumulated.get(key, 0.0) + float(value)

    @property
    def time_averaged_game_stats(self) -> dict:
        if self.step_count == 0:
            return {}
        return {k: v / self.step_count for k, v in self.accumulated.items()}


def oracle_game(prog, o) -> dict:
    """episode_stats["game"] of an oracle env."""
    return stats_dicts(prog, *o.raw_stats(), extra=o.invalid_index_extra())["game"]


def same_f64_dict(got: dict, want: dict, where: str) -> None:
    assert sorted(got) == sorted(want), (where, sorted(set(got) ^ set(want)))
    for k, v in want.items():
        assert np.float64(got[k]).tobytes() == np.float64(v).tobytes(), (where, k, float(got[k]).hex(), float(v).hex())


def load(name):
    """-> (doc: map / seed / set_inventory, expected, traces, program).  rung3_s0 is a scenario of tests/golden/make_golden.py
    (this project's spec, played by the reference engine over the golden's whole trace); the others are reference configs."""
    if name == "rung3_s0":
        want = json.load(open(os.path.join(HERE, "golden", f"time_avg_{name}.json")))
        want["time_averaged_game_stats"] = {k: float.fromhex(v) for k, v in want["time_averaged_game_stats"].items()}
        z = np.load(os.path.join(HERE, "golden", "rung3_s0.npz"))
        prog = hp.compile_scenario("rung3", hp.SCENARIOS["rung3"][0](), *z["class_map"].shape)
        return {"class_map": z["class_map"], "seed": 0, "set_inventory": [], "runs_to_the_end": False}, want, z, prog
    doc = json.load(open(os.path.join(HERE, "golden", f"ref_{name}.json")))
    want = json.load(open(os.path.join(HERE, "golden", f"time_avg_{name}.json")))
    want["time_averaged_game_stats"] = {k: float.fromhex(v) for k, v in want["time_averaged_game_stats"].items()}
    z = np.load(os.path.join(HERE, "golden", f"ref_{name}.npz"))
    cfg = ref_tree.load(doc["config"])
    prog = from_reference.compile_reference_config(cfg, len(doc["map"]), len(doc["map"][0]))
    doc.update(class_map=prog.class_map(doc["map"]), runs_to_the_end=True)
    return doc, want, z, prog


def test_some_fixture_key_appears_after_the_first_step():
    """Key-existence timing is exercised: a key the game dict does not hold after step 1 is averaged over ALL steps."""
    assert any(json.load(open(os.path.join(HERE, "golden", f"time_avg_{n}.json")))["late_keys"] for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_time_averages_equal_the_reference_handler(name):
    doc, want, z, prog = load(name)
    o = op.OracleSim(prog, doc["class_map"], doc["seed"])
    o.reinit_buffers()
    h = TimeAveragedStats()
    for t in range(want["steps_played"]):
        for when, agent_id, inv in doc["set_inventory"]:
            if when == t:
                o.set_inventory(agent_id, dict(map(tuple, inv)))
        o.step(z["actions"][t], z["vibe_actions"][t])
        h.on_step(oracle_game(prog, o))
        if t == 0:
            assert sorted(oracle_game(prog, o)) == want["keys_after_step_1"]
    s = o.snapshot()
    assert not doc["runs_to_the_end"] or s["truncations"].all() or s["terminals"].all()
    same_f64_dict(h.time_averaged_game_stats, want["time_averaged_game_stats"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_engine_log_record_equals_the_reference_handler(name):
    from mettagrid_amd.engine import BatchedMettaGrid
    doc, want, z, prog = load(name)
    eng = BatchedMettaGrid(prog, doc["class_map"][None], [doc["seed"]], buffers="host", specialize=False)
    eng.set_episode_stats(True, log_capacity=2)
    eng.set_time_averages(True, log_capacity=2)
    for t in range(want["steps_played"]):
        for when, agent_id, inv in doc["set_inventory"]:
            if when == t:
                eng.set_inventory(0, agent_id, dict(map(tuple, inv)))
        eng.actions[:] = z["actions"][t]
        eng.vibe_actions[:] = z["vibe_actions"][t]
        eng.step()
    assert not doc["runs_to_the_end"] or eng.truncations.all() or eng.terminals.all()
    (mid,) = eng.time_averages([0])                      # the handler's property, read before the episode is finished
    same_f64_dict(mid, want["time_averaged_game_stats"], f"{name} property")
    eng.record_episodes([1])
    (rec,), dropped = eng.drain_time_average_log()
    assert dropped == 0 and not rec["partial"] and rec["steps"] == rec["ta_steps"] == want["steps_played"]
    same_f64_dict(rec["time_averaged_game_stats"], want["time_averaged_game_stats"], f"{name} record")
    tot = eng.drain_time_averages()
    assert tot["episodes"] == 1 and tot["partial"] == 0
    same_f64_dict(tot["sum"], want["time_averaged_game_stats"], f"{name} totals")   # one episode: the sums are its values
    eng.close()
