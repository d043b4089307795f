"""lii_pose_refine and the communicator.

  * a communicator of MORE than one rank: both forms refuse with LII_ERR_STATE and write nothing (two ranks on one device over the
    mailbox transport, each a child process: tests/pose_refine_rank_worker.py);
  * a communicator of ONE rank (attached as the other suites attach it, over RCCL) does not stand in the way: the same bytes as before.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_score_cases as psc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STATE = -5  # LII_ERR_STATE


def test_refused_with_two_ranks_attached(tmp_path):
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=1024, max_map_points=1024)
    uid = r.comm_unique_id().hex()
    r.close()
    world, procs, outs = 2, [], []
    for rank in range(world):
        outs.append(str(tmp_path / f"rank{rank}.npz"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "pose_refine_rank_worker.py"), str(rank), str(world), uid, "mailbox", outs[-1]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace"))
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    for o in outs:
        got = dict(np.load(o))
        assert str(got["transport"]) == "mailbox" and int(got["n"]) == 500
        assert (int(got["rc_h"]), int(got["rc_d"])) == (STATE, STATE)
        assert bool(got["host_untouched"]) and bool(got["dev_untouched"])


def test_served_with_a_one_rank_communicator(oracle, small_world):
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    scan = psc.tiny_scan(small_world)[:2000]
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.scan_upload(scan)
    assert reg.downsample_skip() == len(scan)
    _, _, R, p = psc.parity_poses(small_world)[0]
    base = lii.State(psc.state_at(oracle, R[0], p[0]))
    before = reg.pose_refine(base, (R[:5], p[:5]))
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    with_comm = reg.pose_refine(base, (R[:5], p[:5]))
    reg.comm_destroy()
    after = reg.pose_refine(base, (R[:5], p[:5]))
    assert before["effect_num"][0] > 0.9 * len(scan)
    for got in (with_comm, after):
        assert np.array_equal(got.view(np.uint8), before.view(np.uint8))
    reg.close()
