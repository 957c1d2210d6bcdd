"""bench.py --dump-outputs: the layout and size of what it writes (host stand-in for the env groups), and on the GPU that
the same arguments give the same arrays while --steps changes them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Engine:
    def __init__(self, rows0: int, rows: int) -> None:
        self.r = np.arange(rows0, rows0 + rows)

    def action_success(self):
        return self.r % 3 == 0

    def episode_rewards(self):
        return (self.r * 0.5).astype(np.float32)


class _Groups:
    """The attributes of mettagrid_amd.groups.EnvGroups that dump_outputs reads, on the host.  The observation rows are a
    broadcast view (row r holds r % 251 in every byte), so that full-size shapes cost no memory."""

    def __init__(self, E: int, A: int, T: int, G: int) -> None:
        self.E, self.A, self.T = E, A, T
        rows = E * A
        self.obs = (torch.arange(rows, dtype=torch.int64) % 251).to(torch.uint8)[:, None, None].expand(rows, T, 3)
        self.rewards = torch.arange(rows, dtype=torch.float32) * 0.25
        self.terminals = torch.arange(rows) % 5 == 0
        self.truncations = torch.arange(rows) % 7 == 0
        self.engines = [_Engine(g * rows // G, rows // G) for g in range(G)]

    def sync(self) -> None:
        pass


@pytest.mark.parametrize("E,A,T,G", [(64, 16, 200, 1), (96, 6, 120, 2), (65536, 16, 200, 1), (65536, 64, 256, 1)])
def test_dump_layout_and_size(E, A, T, G, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    grp = _Groups(E, A, T, G)
    bench.dump_outputs(grp, str(tmp_path))
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(f.endswith(".npy") for f in os.listdir(tmp_path))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())

    row_envs = files["row_envs"].astype(np.int64) if "row_envs" in files else np.arange(E)
    assert ("row_envs" in files) == (E * A > bench.DUMP_ROWS)
    rows = (row_envs[:, None] * A + np.arange(A)).ravel()
    assert np.array_equal(files["rewards"], rows * 0.25)
    assert np.array_equal(files["terminals"], (rows % 5 == 0).astype(np.float32))
    assert np.array_equal(files["truncations"], (rows % 7 == 0).astype(np.float32))
    assert np.array_equal(files["action_success"], (rows % 3 == 0).astype(np.float32))
    assert np.array_equal(files["episode_rewards"], rows * 0.5)

    obs_envs = files["obs_envs"].astype(np.int64)
    assert len(obs_envs) >= 1 and np.all(np.diff(obs_envs) > 0) and obs_envs[-1] < E
    obs_rows = (obs_envs[:, None] * A + np.arange(A)).ravel()
    assert files["obs_sample"].shape == (len(obs_rows), T, 3)
    assert np.array_equal(files["obs_sample"][:, 0, 0], obs_rows % 251)

    again = tmp_path / "again"
    bench.dump_outputs(grp, str(again))   # the sample is fixed: same envs every run
    assert np.array_equal(np.load(again / "obs_envs.npy"), files["obs_envs"])


def _bench_dump(out_dir, steps: int) -> dict:
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "256", "--steps", str(steps),
            "--warmup", "2", "--no-cpu", "--no-extras", "--dump-outputs", str(out_dir)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_dump_repeats_and_follows_steps(tmp_path):
    a, b, c = _bench_dump(tmp_path / "a", 3), _bench_dump(tmp_path / "b", 3), _bench_dump(tmp_path / "c", 4)
    assert a.keys() == b.keys() == c.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["episode_rewards"], c["episode_rewards"]) or not np.array_equal(a["obs_sample"], c["obs_sample"])
