"""bench.py as the driver launches it for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N`.
On a single-GPU box the ranks share device 0 (LII_BENCH_ONE_DEVICE=1: rendezvous over gloo, the node-local mailbox transports -
RCCL refuses two ranks on one device); with two or more visible devices the real arrangement runs as well (one device per rank,
rendezvous over RCCL, every transport timed).  Checked: the JSON line the driver parses is there and complete, every transport that
can run here was timed, and the sharded job's final state is the single-rank job's within the suite's pose tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --full: the other transports and partitions, roofline.scan and the live traffic passes are measured only there
COMMON = ["--full", "--steps", "20", "--warmup", "5", "--prime", "10", "--long-steps", "0", "--no-cpu-baseline", "--no-pipeline", "--no-calibration",
          "--no-live-traffic", "--workload", "vlp16"]


def _line(out):
    rows = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(rows) == 1, out[-3000:]  # rank 0 prints ONE line
    return json.loads(rows[0])


def _single():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + COMMON, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return _line(p.stdout)


def _sharded(n, port, one_device, partition="index"):
    env = dict(os.environ)
    if one_device:
        env["LII_BENCH_ONE_DEVICE"] = "1"
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--partition", partition] + COMMON,
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    return _line(p.stdout)


def _check(d, one, n, expect_transports):
    assert d["n_gpus"] == n and d["steps"] == 20 and d["value"] > 0 and d["unit"] == "scans/s"
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    for t in expect_transports:
        assert t in d["transports"] and d["transports"][t].get("value", 0) > 0, d["transports"]
    assert d["config"]["transport"] == expect_transports[0]
    assert d["config"]["transport_why"]
    assert np.isfinite(d["roofline"]["scan"]["frac"]) and d["roofline"]["scan"]["frac"] > 0
    # the same stream, the same steps: the sharded job ends where the single-rank job ends (91 sums re-associated)
    assert np.max(np.abs(np.array(d["last_state_pose"]) - np.array(one["last_state_pose"]))) <= 1e-6
    assert d["config"]["avg_iterations"] == one["config"]["avg_iterations"]
    # both splits of the cloud were timed on the first transport (`value` with config.partition), and the split by voxel was really one
    for part in ("index", "voxel"):
        assert d["partitions"][part].get("value", 0) > 0, d["partitions"]
    assert "split by voxel" in d["partitions"]["voxel"]["describe"] and "split by index" in d["partitions"]["index"]["describe"]
    assert d["partitions"][d["config"]["partition"]]["value"] == d["value"]


@pytest.mark.parametrize("partition", ["index", "voxel"])
def test_bench_two_ranks_on_one_device(partition):
    one = _single()
    d = _sharded(2, 29611 + (partition == "voxel"), one_device=True, partition=partition)
    _check(d, one, 2, ["mailbox", "mailbox_host"])
    assert d["config"]["rccl_ranks"] == 0 and d["config"]["partition"] == partition


def test_bench_four_ranks_on_one_device():
    """Four processes time-sharing one device: wavefronts are preempted in the middle of kernels, which stretches every window between
    two dependent loads - the arrangement that exposed a torn read of a voxel-filter slot in round 4 (VhSlot, lii_scan.hip)."""
    one = _single()
    d = _sharded(4, 29615, one_device=True, partition="voxel")
    _check(d, one, 4, ["mailbox", "mailbox_host"])


def test_bench_two_ranks_on_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    one = _single()
    d = _sharded(2, 29613, one_device=False)
    _check(d, one, 2, ["mailbox", "rccl", "mailbox_host"])
    assert d["transports"]["rccl"]["rccl_ranks"] == 2


def test_single_rank_line_measures_its_hbm_traffic_in_the_run():
    """roofline.traffic of a single-rank line: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) around a short child run of the same
    command, per executed launch of the search kernel - or, where no profiler can run, the committed passes, saying so and why."""
    flags = [f for f in COMMON if f != "--no-live-traffic"][:-2] + ["--workload", "stream100k", "--kernel-profile-steps", "0"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    r = _line(p.stdout)["roofline"]
    assert r["traffic"] is not None and r["traffic_source"]
    if r["traffic_source"].startswith("measured in this run"):
        # the search reads every query and the map once and writes five neighbours per query: the counters must land near the
        # algorithmic bytes (22.6 MB measured against 25.1 MB: the L2 keeps part of the map across the two passes of a scan)
        assert 0.5 * r["alg_bytes_per_launch"] < r["traffic"] < 1.5 * r["alg_bytes_per_launch"], r
    else:
        assert "not measured in this run" in r["traffic_source"], r
