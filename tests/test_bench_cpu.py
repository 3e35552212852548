"""bench.py's launcher and argument logic on the CPU: `--gpus N` either starts N ranks
or fails loudly, a torch.distributed environment that disagrees with --gpus exits non-zero, and the C4 /
strong-scaling shard plan covers every pair once."""
import json
import os
import subprocess
import sys
import types

import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def run_bench(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_world_size_mismatch_exits_2():
    r = run_bench(["--gpus", "4", "--cpu-sample", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 4" in json.loads(r.stdout.strip().splitlines()[-1])["error"]


def test_gpus_without_enough_devices_fails_loudly():
    # this container has no GPU: `--gpus 2` must not fall back to one rank
    r = run_bench(["--gpus", "2", "--cpu-sample", "0"], {})
    assert r.returncode == 2
    assert "needs 2 GPUs" in json.loads(r.stdout.strip().splitlines()[-1])["error"]


def test_launcher_starts_n_ranks(monkeypatch):
    import torch
    seen = {}

    def fake_run(cmd, env):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=0)

    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--total-pairs", "64"])
    args = types.SimpleNamespace(gpus=8)
    assert bench.launch_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--total-pairs", "64"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_check_world(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert bench.check_world(types.SimpleNamespace(gpus=1)) == (1, 0, 0)
    assert bench.check_world(types.SimpleNamespace(gpus=2)) is None
    monkeypatch.setenv("WORLD_SIZE", "8")
    monkeypatch.setenv("RANK", "3")
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert bench.check_world(types.SimpleNamespace(gpus=8)) == (8, 3, 3)
    with pytest.raises(SystemExit):
        bench.check_world(types.SimpleNamespace(gpus=1))


@pytest.mark.parametrize("total", [64, 65, 7, 1])
def test_strong_scaling_shards(total):
    for world in (1, 2, 4, 8):
        spans = [bench.shard(total, world, r) for r in range(world)]
        assert sum(c for _, c in spans) == total
        assert [s for s, _ in spans] == [sum(c for _, c in spans[:r]) for r in range(world)]


def test_make_batch_renders_synth_bytes():
    """bench.make_batch (forked renderers, shared buffer) against synth.make_batch, in a process of its own
    as in the bench: it forks.  9 pairs on 2 processes (5 + 4), and 7 pairs (too few to fork for 2)."""
    code = ("import bench; from pyorbslam_amd import synth\n"
            "for n in (9, 7):\n"
            "    got = bench.make_batch(n, 5, 160, 120, 2)\n"
            "    assert got.shape == (2 * n, 120, 160) and got.dtype.name == 'uint8'\n"
            "    assert got.tobytes() == synth.make_batch(n, seed0=5, width=160, height=120).tobytes()\n"
            "print('same')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "same", r.stdout[-1000:] + r.stderr[-3000:]


def test_full_and_dump_outputs_are_options():
    r = run_bench(["--gpus", "4", "--full", "--dump-outputs", "unused", "--cpu-sample", "0"],
                  {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2 but --gpus 4" in r.stdout  # parsed; stopped by the world check


def test_dump_outputs_layout(tmp_path):
    """dump_outputs over two stand-in handles (3 + 2 pairs, global pair g = image pair of handle g // 3): every
    pair lands in its row, rows are zero beyond the pair's count, every file is float32 / float64."""
    import numpy as np
    from pyorbslam_amd._lib import KP_DTYPE
    cap = 6

    class Handle:
        kp_cap = cap

        def __init__(self, first):
            self.first = first

        def overflow(self):
            return 0

        def fetch_image(self, i):
            g, side = self.first + i // 2, i % 2
            n = 1 + (2 * g + side) % cap
            k = np.zeros(n, KP_DTYPE)
            k["x"], k["y"], k["octave"] = 100 * g + side + np.arange(n) / 8, g, np.arange(n) % 8
            return k, np.full((n, 32), (10 * g + side) % 251, np.uint8)

        def fetch_stereo(self, p):
            g = self.first + p
            n = 1 + (2 * g) % cap
            return dict(u_right=np.full(n, g + 0.5, np.float32), depth=np.full(n, -1, np.float32),
                        status=np.ones(n, np.int8), match_r=np.arange(n, dtype=np.int32) - 1)

    sh = types.SimpleNamespace(fes=[Handle(0), Handle(3)], counts=[3, 2], n_pairs=5)
    info = bench.dump_outputs(tmp_path / "o", sh)
    got = {p.stem: np.load(p) for p in (tmp_path / "o").iterdir()}
    assert info["pairs"] == 5 and info["bytes"] == sum(a.nbytes for a in got.values())
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["sample_pairs"].tolist() == [0, 1, 2, 3, 4] and got["overflow"].tolist() == [0, 0]
    assert got["keypoints"].shape == (5, 2, cap, 6) and got["descriptors"].shape == (5, 2, cap, 32)
    for g in range(5):
        for side in (0, 1):
            n = 1 + (2 * g + side) % cap
            assert got["n_keypoints"][g, side] == n
            assert got["keypoints"][g, side, :n, 0].tolist() == [100 * g + side + j / 8 for j in range(n)]
            assert got["keypoints"][g, side, :n, 5].tolist() == [j % 8 for j in range(n)]
            assert (got["descriptors"][g, side, :n] == 10 * g + side).all()
            assert not got["keypoints"][g, side, n:].any() and not got["descriptors"][g, side, n:].any()
        n = 1 + (2 * g) % cap
        assert (got["u_right"][g, :n] == g + 0.5).all() and (got["depth"][g, :n] == -1).all()
        assert got["match_r"][g, :n].tolist() == list(range(-1, n - 1)) and not got["status"][g, n:].any()
    # a larger shard: a fixed sample, the same on every call
    big = types.SimpleNamespace(fes=[Handle(0)], counts=[100], n_pairs=100)
    a = bench.dump_outputs(tmp_path / "a", big)
    bench.dump_outputs(tmp_path / "b", big)
    sa, sb = np.load(tmp_path / "a" / "sample_pairs.npy"), np.load(tmp_path / "b" / "sample_pairs.npy")
    assert a["pairs"] == bench.DUMP_MAX_PAIRS == len(set(sa.tolist())) and np.array_equal(sa, sb)
    assert np.load(tmp_path / "a" / "n_keypoints.npy")[:, 0].tolist() == [1 + (2 * int(g)) % cap for g in sa]


def test_stamped_lookup(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", tmp_path)
    (tmp_path / "profiles").mkdir()
    (tmp_path / "profiles" / "x.json").write_text(json.dumps({"w": {"detect": 1.0}, "w_meta": {"build_id": "abc"}}))
    v, src = bench.stamped("x.json", "w", "abc")
    assert v == {"detect": 1.0} and "abc" in src
    v, src = bench.stamped("x.json", "w", "def")
    assert v is None and "dropped" in src
    v, src = bench.stamped("x.json", "other", "abc")
    assert v is None
