"""The bench's N > 1 path on the GPU box: `bench.py --gpus 2` started as a fresh
process goes through its own launcher (torch.distributed.run child, two ranks sharing the one GPU with the
gloo backend, ORBFE_DIST_BACKEND=gloo), and its JSON line must report two ranks, a clean parity sample and
correct gathered records for the weak-scaling step and for C4."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_two_ranks_through_the_launcher():
    env = dict(os.environ, ORBFE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--pairs", "8", "--steps", "3", "--warmup", "1",
           "--full", "--cpu-sample", "0", "--no-c3", "--roofline-steps", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["total_pairs_per_step"] == 16
    assert out["parity_failures"] == 0 and out["overflow"] == 0 and out["parity_checked_pairs"] == 16
    assert out["with_gather"]["record_check"] is True
    assert out["with_gather"]["pairs_gathered"] == 16
    # every gathered record unpacked on rank 0 and checked against its sender's digest
    assert out["with_gather"]["records_verified"] == 16
    assert out["c4_strong"]["with_gather"]["record_check"] is True
    assert out["c4_strong"]["with_gather"]["records_verified"] == 64
    assert out["c4_strong"]["pairs_per_gpu"] == 32
    assert out["host_fed"]["record_check"] is True


DUMPED = {"sample_pairs", "overflow", "n_keypoints", "keypoints", "descriptors", "u_right", "depth", "status",
          "match_r"}
FULL_ONLY = ("parity_checked_pairs", "c4_strong", "c4_rank_share", "c5_euroc", "host_fed", "c3_frame",
             "stage_ms_standalone_step", "roofline", "valu_roofline")


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run reports only the timed steps (nothing of --full), and --dump-outputs writes what those
    steps left in the handles: 8 pairs as 3 handles (3 + 3 + 2) against the same 8 pairs through one handle
    in this process, value for value."""
    import numpy as np
    import torch
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--pairs", "8", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "pairs/s" and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(8 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in out] and out["cpu_baseline"] is None
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(got) == DUMPED
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["sample_pairs"].tolist() == list(range(8)) and not got["overflow"].any()

    fe = StereoFrontEnd(max_pairs=8, lanes=1)
    fe.enqueue(torch.from_numpy(synth.make_batch(8)).cuda(), 8)
    torch.cuda.synchronize()
    for p in range(8):
        for side in (0, 1):
            k, d = fe.fetch_image(2 * p + side)
            n = int(got["n_keypoints"][p, side])
            assert n == len(k) > 0
            want = np.stack([k[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave")], 1)
            assert np.array_equal(got["keypoints"][p, side, :n], want) and not got["keypoints"][p, side, n:].any()
            assert np.array_equal(got["descriptors"][p, side, :n], d.astype(np.float32))
        st = fe.fetch_stereo(p)
        n = int(got["n_keypoints"][p, 0])
        for name in ("u_right", "depth", "status", "match_r"):
            assert np.array_equal(got[name][p, :n], st[name].astype(np.float32)), (p, name)
        assert (got["status"][p] > 0).any()


def test_c4_eight_ranks_through_the_launcher():
    """C4's real 8-way shape end to end — `bench.py --gpus 8 --total-pairs 64` through its own
    launcher, 8 ranks sharing the one GPU with gloo: the 8-rank shard plan (8 pairs each), the 8-sender
    rank-0 buffer, the compact unpack of 64 records, parity of every rank's pairs."""
    env = dict(os.environ, ORBFE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "8", "--total-pairs", "64", "--pairs", "8", "--steps", "3",
           "--warmup", "1", "--full", "--cpu-sample", "0", "--no-c3", "--no-host-fed", "--roofline-steps", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["scaling"] == "strong"
    assert out["config"]["total_pairs_per_step"] == 64 and out["config"]["pairs_per_step_per_gpu"] == 8
    assert out["parity_failures"] == 0 and out["overflow"] == 0 and out["parity_checked_pairs"] == 64
    g = out["c4_strong"]["with_gather"]
    assert g["record_check"] is True and g["pairs_gathered"] == 64
    assert g["records_verified"] == 64 and g["padded_rows_zero"] == 0
    assert out["with_gather"]["record_check"] is True and out["with_gather"]["records_verified"] == 64
    assert out["with_gather"]["bytes_to_rank0"] == 64 * g["record_bytes"]
